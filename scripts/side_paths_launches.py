"""The kernel launches of the list, range and bitmap searches, for comparing two builds of the library (EHX_LIB selects
one): the kernel names of one short run, ordered by start time, must be the same before and after a change of host code.

  run   (no arguments; under the profiler, in a fresh process per library)
          rocprofv3 --kernel-trace -d DIR -o trace -- python scripts/side_paths_launches.py
        one 20 000 x 128 cosine flat space (fill_synthetic; above the int8 engine's 16 384-row floor), 64 queries, k = 10,
        one call each of range_device (radii = every query's 5th nearest distance: a handful of rows per query),
        knn_masked_device under an all-ones bitmap (scan route) and under a 500-row bitmap (exact route), and
        knn_among_device with a 100-id shared list.
  list  python scripts/side_paths_launches.py --list DIR > listing.txt
        the kernel names of the trace under DIR (rocpd database), one per line, ordered by start time."""
import ctypes as C
import glob
import os
import sqlite3
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run():
    import numpy as np
    import torch
    import embeddinghub_amd as ehx
    from embeddinghub_amd import _lib
    from embeddinghub_amd.space import marshal_mask
    rows, dims, nq, k = 20000, 128, 64, 10
    L = _lib.load()
    sp = ehx.Space.unique("side-launches", dims, metric=ehx.METRIC_COSINE, initial_capacity=rows)
    sp.fill_synthetic(ehx.SEED_CORPUS, 0, rows, True)
    assert sp.scan_engine() == "i8"
    st = torch.cuda.current_stream().cuda_stream
    q = torch.empty((nq, dims), dtype=torch.float32, device="cuda")
    _lib.check(L.ehx_gen_rows_device(C.c_void_p(st), ehx.SEED_QUERY, 0, nq, dims, 1, C.c_void_p(q.data_ptr())))
    ids = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    dist = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    cnt = torch.empty((nq,), dtype=torch.int32, device="cuda")
    tot = torch.empty((nq,), dtype=torch.int64, device="cuda")
    sp.knn_device(q, k, ids, dist, cnt, stream=st)
    torch.cuda.synchronize()
    radius = dist[:, 4].contiguous()
    sp.range_device(q, radius, k, ids, dist, cnt, tot, stream=st)
    torch.cuda.synchronize()
    print("range_device: members per query", tot.cpu().numpy().tolist()[:8], "...")
    for name, allowed in (("all rows", np.ones(rows, dtype=bool)), ("500 rows", np.arange(rows) % (rows // 500) == 0)):
        words, n_bits = marshal_mask(allowed)
        d_mask = torch.tensor(words.view(np.int32), device="cuda")
        sp.knn_masked_device(q, k, d_mask, n_bits, ids, dist, cnt, stream=st)
        torch.cuda.synchronize()
        print("knn_masked_device, %s: checksum %d" % (name, int(ids.sum().item())))
    d_list = torch.arange(0, rows, rows // 100, dtype=torch.int64, device="cuda")[:100].contiguous()
    sp.knn_among_device(q, k, d_list, None, ids, dist, cnt, stream=st)
    torch.cuda.synchronize()
    print("knn_among_device: checksum %d" % int(ids.sum().item()))
    sp.drop()


def listing(d):
    dbs = sorted(glob.glob(os.path.join(d, "**", "*.db"), recursive=True))
    if not dbs:
        sys.exit("no rocpd database under %s" % d)
    c = sqlite3.connect(dbs[0])
    tables = [r[0] for r in c.execute("select name from sqlite_master where type in ('table', 'view')")]
    disp = [t for t in tables if t.startswith("rocpd_kernel_dispatch")][0]
    sym = [t for t in tables if t.startswith("rocpd_info_kernel_symbol")][0]
    for (name,) in c.execute("select s.kernel_name from %s d join %s s on d.kernel_id = s.id order by d.start" % (disp, sym)):
        print(name)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--list":
        listing(sys.argv[2])
    else:
        run()
