"""One sha256 per case of the track path, for comparing two builds of the library bit for bit: run it once with DMX_LIB
pointing at each build, each in a fresh process, and compare the outputs (profiles/track_path_hash_*.txt).

Synthetic 4-source models (seeds 50..53), segment 8000, fixed shifts; three tracks of 30 011, 8 000 and 1 234 samples:
  tracks_planar / tracks_eigen   Context.tracks, max_batch 3, both layouts              (track_ola_kernel)
  tracks_opts                    N = 3, overlap 0.75, copies with different segment counts (track_ola_ens_kernel, tail rows)
  tracks_bag                     Q = 2, general weights, N = 2                           (track_ola_bag_kernel)
  tracks_bag_diagonal            the 4-model diagonal bag                                (track_ola_bag_kernel, one model per stem)
  tracks_pcm                     S16 / rescale                                           (planar slot + pcm.hip)

    DMX_LIB=path/to/libdemucs_hip.so python tools/track_path_hash.py
"""
import hashlib
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from demucs_cpp_amd import binding as dmx  # noqa: E402
from demucs_cpp_amd.weights import write_synthetic_model  # noqa: E402

SEG = 8000
LENGTHS = (30011, 8000, 1234)


def digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def main():
    rng = np.random.default_rng(7)
    audios = [(0.1 * rng.standard_normal((2, n))).astype(np.float32) for n in LENGTHS]
    with tempfile.TemporaryDirectory() as d:
        paths = [os.path.join(d, f"ggml-model-htdemucs-4s-f16-{i}.bin") for i in range(4)]
        for i, p in enumerate(paths):
            write_synthetic_model(p, 4, 50 + i)
        models = [dmx.Model(p, 0) for p in paths]
        ctx = dmx.Context(models[0], SEG, 3)
        one = [4033, 12436, 5427]
        print("tracks_planar", digest(ctx.tracks(audios, one)))
        print("tracks_eigen", digest(ctx.tracks(audios, one, layout=dmx.LAYOUT_EIGEN)))
        ens = np.array([[0, 9000, 22049], [22049, 0, 11000], [5, 21000, 10000]])
        counts = {dmx.track_geometry(SEG, LENGTHS[0], int(s), 0.75)[1] for s in ens[0]}
        assert len(counts) == 3, counts  # the copies of the long track differ in their segment counts
        print("tracks_opts", digest(ctx.tracks_opts(audios, 3, 0.75, ens)))
        w = np.array([[1.0, 0.5, 0.0, 2.0], [0.25, 0.5, 1.0, 0.0]], np.float32)
        bag = np.array([[[0, 22049], [9000, 3]], [[22049, 0], [1, 11000]], [[5, 21000], [10000, 7]]])
        print("tracks_bag", digest(ctx.tracks_bag(models[:2], audios, w, 2, 0.25, bag)))
        diag = np.array([[[4033], [12436], [5427], [6865]]] * 3)
        print("tracks_bag_diagonal", digest(ctx.tracks_bag(models, audios, shift_offsets=diag)))
        outs, peaks = ctx.tracks_pcm(audios, dmx.OutputSpec(dmx.PCM_S16, dmx.CLIP_RESCALE), shift_offsets=np.array(one).reshape(3, 1))
        print("tracks_pcm", digest([o for t in outs for o in t] + peaks))
        ctx.close()
        for m in models:
            m.close()


if __name__ == "__main__":
    main()
