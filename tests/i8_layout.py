"""The layouts of the int8 filter scan in numpy, restated from the comments of csrc/ehx_kernels.h and csrc/k_misc.hip (not
by calling the library): where an element of the scan copy, of a query tile and of the sample pass's dump lives, which
lane group a tile position belongs to, where a rank of the tile ordering is stored, and how a pool key decodes."""
import numpy as np

TILE = 256          # rows (and queries) per tile
STAGE = 64          # bytes (= k-values) per stage row
POOL_CAP = 4096     # kPoolCap
SAMPLE_TILES = 8    # the sample pass's window
SWIZZLE = (0, 2, 3, 1)   # chunk swizzle by (row >> 2) & 3: the 16-byte chunk c of a row sits at physical chunk c ^ SWIZZLE[...]


def _swz(rr, table):
    return np.asarray(table, dtype=np.int64)[(rr >> 2) & 3]


def scan8_index(row, col, ld8, table=SWIZZLE):
    """byte index of element (row, col) of the scan copy: tiles of 256 rows, stages of 64 columns, one (tile, stage) block =
    256 rows x 64 B, blocks ordered [tile][stage], the row's four 16-byte chunks swizzled"""
    row, col = np.asarray(row, dtype=np.int64), np.asarray(col, dtype=np.int64)
    tile, rr, kt, cc = row >> 8, row & 255, col >> 6, col & 63
    chunk = (cc >> 4) ^ _swz(rr, table)
    return ((tile * (ld8 >> 6) + kt) * 256 + rr) * 64 + chunk * 16 + (cc & 15)


def scanq8_index(row, stage, cc, ld8, table=SWIZZLE):
    """byte index of column cc (< 64) of stage block `stage` of query `row`: the same blocks, [q_tile][stage], ld8 / 64 + 3
    blocks per query tile — block kts + j (j < 3) repeats stage j mod kts"""
    row, stage, cc = np.asarray(row, dtype=np.int64), np.asarray(stage, dtype=np.int64), np.asarray(cc, dtype=np.int64)
    tile, rr = row >> 8, row & 255
    chunk = (cc >> 4) ^ _swz(rr, table)
    return ((tile * ((ld8 >> 6) + 3) + stage) * 256 + rr) * 64 + chunk * 16 + (cc & 15)


def scanq8_bytes(q_rows, ld8):
    return (q_rows >> 8) * ((ld8 >> 6) + 3) * 256 * 64


def scan8_dump_index(q, row, n_s):
    """element index of (query q, sample row `row`) in the dump of a sample of n_s rows: blocks of 16 queries x 16 rows, a
    query's 16 rows contiguous"""
    q, row = np.asarray(q, dtype=np.int64), np.asarray(row, dtype=np.int64)
    return ((((q >> 4) * (n_s >> 4)) + (row >> 4)) << 8) + ((q & 15) << 4) + (row & 15)


def i8_group_of_pos(p):
    """lane group (g = 4 wr + (l >> 4)) of tile position p = 128 wr + 16 rb + 4 q' + r"""
    p = np.asarray(p, dtype=np.int64)
    return ((p >> 7) << 2) | ((p >> 2) & 3)


def i8_pos_of_rank(rank):
    """tile position of rank `rank` of the tile ordering: ranks 32 g .. 32 g + 31 fill lane group g"""
    rank = np.asarray(rank, dtype=np.int64)
    g, m = rank >> 5, rank & 31
    return (g >> 2) * 128 + (m >> 2) * 16 + (g & 3) * 4 + (m & 3)


def f32_to_ordered(f):
    """(score, id) keys: unsigned order of the 32 bits == order of the floats"""
    u = np.asarray(f, dtype=np.float32).view(np.uint32)
    return u ^ np.where(u >> 31 != 0, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def ordered_to_f32(o):
    o = np.asarray(o, dtype=np.uint32)
    return (o ^ np.where(o >> 31 != 0, np.uint32(0x80000000), np.uint32(0xFFFFFFFF))).view(np.float32)


def decode_key(key):
    """pool key -> (row id u32, score f32)"""
    key = np.asarray(key, dtype=np.uint64)
    return (key & np.uint64(0xFFFFFFFF)).astype(np.uint32), ordered_to_f32((key >> np.uint64(32)).astype(np.uint32))


def delayout_x8(raw, n_rows, ld8, table=SWIZZLE):
    """raw scan copy bytes -> codes [n_rows][ld8] by POSITION"""
    idx = scan8_index(np.arange(n_rows)[:, None], np.arange(ld8)[None, :], ld8, table)
    return np.asarray(raw).view(np.int8)[idx]


def layout_x8(codes, ld8, table=SWIZZLE):
    n = codes.shape[0]
    raw = np.zeros(n * ld8, dtype=np.int8)
    raw[scan8_index(np.arange(n)[:, None], np.arange(ld8)[None, :], ld8, table)] = codes
    return raw


def delayout_q8(raw, nq, ld8, table=SWIZZLE):
    """raw query tiles -> codes [nq][ld8] (the stages proper, not the three repeated blocks)"""
    col = np.arange(ld8)[None, :]
    idx = scanq8_index(np.arange(nq)[:, None], col >> 6, col & 63, ld8, table)
    return np.asarray(raw).view(np.int8)[idx]


def layout_q8(codes, q_rows, ld8, table=SWIZZLE):
    """codes [nq][ld8] -> the raw query tiles of q_rows rows, padding queries zero, with the three repeated blocks"""
    nq, kts = codes.shape[0], ld8 >> 6
    raw = np.zeros(scanq8_bytes(q_rows, ld8), dtype=np.int8)
    col = np.arange(ld8)[None, :]
    rows = np.arange(nq)[:, None]
    raw[scanq8_index(rows, col >> 6, col & 63, ld8, table)] = codes
    for j in range(3):
        src = (j % kts) * 64 + np.arange(64)[None, :]
        raw[scanq8_index(rows, kts + j, np.arange(64)[None, :], ld8, table)] = codes[:, src[0]]
    return raw
