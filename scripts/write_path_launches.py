"""The kernel launches of the write path, for comparing two builds of the library (EHX_LIB selects one): the kernel names of
one short run, ordered by start time, must be the same before and after a change of host code.

  run   (no arguments; under the profiler, in a fresh process per library)
          rocprofv3 --kernel-trace -d DIR -o trace -- python scripts/write_path_launches.py
        one 20 000 x 128 cosine flat space (above the int8 engine's 16 384-row floor) filled by the generator in two calls
        (12 000 + 8 000), then one 8 192-row append from host memory, one 8 192-row append from device memory, and one
        3-row batch that rewrites two known keys (the exclusive path); one 2 000 x 64 L2 graph space (M = 8), filled by the
        generator, then one host batch of 64 rows that rewrites one known key (replayed row by row).
  list  python scripts/write_path_launches.py --list DIR > listing.txt
        the kernel names of the trace under DIR (rocpd database), one per line, ordered by start time."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scripts.side_paths_launches import listing  # noqa: E402


def run():
    import numpy as np
    import torch
    import embeddinghub_amd as ehx
    rows, dims, chunk = 20000, 128, 8192
    rng = np.random.default_rng(5)
    sp = ehx.Space.unique("write-launches", dims, metric=ehx.METRIC_COSINE, initial_capacity=rows + 2 * chunk + 1)
    sp.fill_synthetic(ehx.SEED_CORPUS, 0, 12000, True)
    sp.fill_synthetic(ehx.SEED_CORPUS, 12000, rows - 12000, True)
    assert sp.scan_engine() == "i8"
    Y = rng.standard_normal((2 * chunk + 3, dims)).astype(np.float32)
    sp.set_batch(["h%d" % i for i in range(chunk)], Y[:chunk])
    sp.set_batch_device(["d%d" % i for i in range(chunk)], torch.from_numpy(Y[chunk:2 * chunk]).cuda())
    sp.set_batch(["h7", "fresh", "123"], Y[2 * chunk:])   # a keyed row, a fresh key, a generated row
    assert len(sp) == rows + 2 * chunk + 1
    print("flat: %d rows, checksum %.6f" % (len(sp), float(sp.get("fresh").sum())))
    sp.drop()
    g_rows, g_dims = 2000, 64
    g = ehx.Space.unique("write-launches-g", g_dims, metric=ehx.METRIC_L2SQ, mode=ehx.MODE_GRAPH, M=8, ef_construction=40, seed=7)
    g.fill_synthetic(ehx.SEED_CORPUS, 0, g_rows, True)
    Z = rng.standard_normal((64, g_dims)).astype(np.float32)
    g.set_batch(["g%d" % i for i in range(63)] + ["17"], Z)
    assert len(g) == g_rows + 63
    print("graph: %d rows, entry point %d" % (len(g), g.graph_export()[3]))
    g.drop()


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--list":
        listing(sys.argv[2])
    else:
        run()
