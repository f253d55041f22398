"""The layouts of the fp16 filter scan in numpy, restated from the comments of csrc/ehx_kernels.h and csrc/k_flat16.hip (not
by calling the library): where a half of the scan copy and of a query tile lives, the tail padding, the sample pass's dump,
the (score, id) keys and which rows a published list covers."""
import numpy as np

from i8_layout import f32_to_ordered, ordered_to_f32  # noqa: F401  (the same key order as the int8 pools)

TILE = 256            # rows (and queries) per tile of the fp16 scan
TILE_F32 = 128        # rows per tile of the fp32 scan
STAGE = 32            # halves per stage row (64 bytes)
SAMPLE_TILES = 8      # the sample pass's window
TAIL_PAD = 3 * 256 * 32   # halves behind the last tile: three stage blocks (DMA read-ahead)
ROWP_PAD = 512        # row parameters behind the last row: two tiles
LISTS_PER_CHUNK = 2   # one published list per wave row
KEY_INF = np.uint64(0xFFFFFFFFFFFFFFFF)
SWIZZLE = (0, 1, 2, 3)    # the 16-byte chunk c of row r sits at physical chunk c ^ SWIZZLE[(r >> 2) & 3]


def ld16_of(d):
    """row stride in halves: a whole number of LDS ring revolutions (4 stages of 32)"""
    return (d + 127) // 128 * 128


def _swz(rr, table):
    return np.asarray(table, dtype=np.int64)[(rr >> 2) & 3]


def scan16_index(row, col, ld16, table=SWIZZLE):
    """index (in halves) of element (row, col): tiles of 256 rows, stages of 32 columns, one (tile, stage) block = 256 rows
    x 64 B, blocks ordered [tile][stage], the row's four 16-byte chunks swizzled"""
    row, col = np.asarray(row, dtype=np.int64), np.asarray(col, dtype=np.int64)
    tile, rr, kt, cc = row >> 8, row & 255, col >> 5, col & 31
    chunk = (cc >> 3) ^ _swz(rr, table)
    return ((tile * (ld16 >> 5) + kt) * 256 + rr) * 32 + chunk * 8 + (cc & 7)


def scanq16_index(row, stage, cc, ld16, table=SWIZZLE):
    """index of column cc (< 32) of stage block `stage` of query `row`: the same blocks, [q_tile][stage], ld16 / 32 + 3 blocks
    per query tile — block kts + j (j < 3) repeats stage j"""
    row, stage, cc = np.asarray(row, dtype=np.int64), np.asarray(stage, dtype=np.int64), np.asarray(cc, dtype=np.int64)
    tile, rr = row >> 8, row & 255
    chunk = (cc >> 3) ^ _swz(rr, table)
    return ((tile * ((ld16 >> 5) + 3) + stage) * 256 + rr) * 32 + chunk * 8 + (cc & 7)


def scanq16_halves(q_rows, ld16):
    return (q_rows >> 8) * ((ld16 >> 5) + 3) * 256 * 32


def x16_halves(cap, ld16):
    return cap * ld16 + TAIL_PAD


def delayout_x16(raw, n_rows, ld16, table=SWIZZLE):
    """raw scan copy (u16) -> halves [n_rows][ld16]"""
    idx = scan16_index(np.arange(n_rows)[:, None], np.arange(ld16)[None, :], ld16, table)
    return np.asarray(raw).view(np.uint16)[idx].view(np.float16)


def layout_x16(halves, cap, ld16, table=SWIZZLE):
    """halves [n][ld16] -> the raw scan copy of `cap` rows with its tail padding"""
    n = halves.shape[0]
    raw = np.zeros(x16_halves(cap, ld16), dtype=np.uint16)
    raw[scan16_index(np.arange(n)[:, None], np.arange(ld16)[None, :], ld16, table)] = np.asarray(halves, dtype=np.float16).view(np.uint16)
    return raw


def delayout_q16(raw, nq, ld16, table=SWIZZLE):
    """raw query tiles -> halves [nq][ld16] (the stages proper, not the three repeated blocks)"""
    col = np.arange(ld16)[None, :]
    idx = scanq16_index(np.arange(nq)[:, None], col >> 5, col & 31, ld16, table)
    return np.asarray(raw).view(np.uint16)[idx].view(np.float16)


def layout_q16(halves, q_rows, ld16, table=SWIZZLE, repeat=True):
    """halves [nq][ld16] -> the raw query tiles of q_rows rows, padding queries zero, with the three repeated blocks"""
    nq, kts = halves.shape[0], ld16 >> 5
    h = np.asarray(halves, dtype=np.float16).view(np.uint16)
    raw = np.zeros(scanq16_halves(q_rows, ld16), dtype=np.uint16)
    col = np.arange(ld16)[None, :]
    rows = np.arange(nq)[:, None]
    raw[scanq16_index(rows, col >> 5, col & 31, ld16, table)] = h
    if repeat:
        for j in range(3):
            raw[scanq16_index(rows, kts + j, np.arange(32)[None, :], ld16, table)] = h[:, j * 32:(j + 1) * 32]
    return raw


def make_key(score, row_id):
    """(ordered(score bits) << 32) | id"""
    return (f32_to_ordered(score).astype(np.uint64) << np.uint64(32)) | np.asarray(row_id, dtype=np.uint64)


def key_score(key):
    return ordered_to_f32((np.asarray(key, dtype=np.uint64) >> np.uint64(32)).astype(np.uint32))


def key_id(key):
    return (np.asarray(key, dtype=np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.int64)


def list_rows(lst, tile0, n_tiles, tiles_per_chunk, tile_rows=TILE):
    """row ids published list `lst` = 2 chunk + wr may hold: the wr-th half of every tile of the chunk"""
    chunk, wr = lst >> 1, lst & 1
    t_lo = tile0 + chunk * tiles_per_chunk
    t_hi = min(t_lo + tiles_per_chunk, tile0 + n_tiles)
    if t_hi <= t_lo:
        return np.zeros(0, dtype=np.int64)
    half = tile_rows // 2
    return (np.arange(t_lo, t_hi, dtype=np.int64)[:, None] * tile_rows + wr * half + np.arange(half, dtype=np.int64)[None, :]).ravel()


def list_of_row(row, tile0, tiles_per_chunk, tile_rows=TILE):
    row = np.asarray(row, dtype=np.int64)
    tile = row // tile_rows
    return ((tile - tile0) // tiles_per_chunk) * 2 + (row % tile_rows) // (tile_rows // 2)
