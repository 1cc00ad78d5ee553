"""Host-side restatement of the draw kernel's thread -> (Philox block, slot) map (csrc/kernels_fullrank_batch.hip, k_fb_eps).  Four waves
(256 threads, tid below; a workgroup is two such groups) draw one block of 64 rows x 32 columns = 512 Philox blocks (block q of a column = its
rows 4 q .. 4 q + 3).  Thread (wave f, lane = column l31 + 32 h) draws blocks 4 f + h and 4 f + 2 + h of column l31 and stores them, as they
come, as its eight slots of fragment f.
Checked here without a GPU: for every fragment lane these are the slots of the earlier map -- one Philox block per thread (q = tid & 15,
column = tid >> 4) through an LDS tile E[column][row], then x[s] = E[l31][16 f + 8 (s >> 2) + 4 h + (s & 3)] -- and the 512 blocks are each
drawn exactly once.  The GPU tests check the numbers; this pins the layout."""
import numpy as np


def tile_of_the_earlier_map():
    """E[column][row] as 512 threads laid it down: the value's identity = (column, Philox block q, element r)."""
    E = np.zeros((32, 64, 3), dtype=np.int64)
    for tid in range(512):
        q, c = tid & 15, tid >> 4
        for r in range(4):
            E[c, 4 * q + r] = (c, q, r)
    return E


def direct_map(tid):
    """(column, [Philox block per half], slots): slot s = 4 b + r holds element r of the thread's block b."""
    f, lane = tid >> 6, tid & 63
    l31, h = lane & 31, lane >> 5
    blocks = [4 * f + 2 * b + h for b in range(2)]
    slots = [(l31, blocks[s >> 2], s & 3) for s in range(8)]
    return l31, blocks, slots


def test_every_fragment_lane_holds_the_slots_of_the_earlier_map():
    E = tile_of_the_earlier_map()
    for tid in range(256):
        f, lane = tid >> 6, tid & 63
        l31, h = lane & 31, lane >> 5
        _, _, slots = direct_map(tid)
        for s in range(8):
            want = tuple(E[l31, 16 * f + 8 * (s >> 2) + 4 * h + (s & 3)])
            assert slots[s] == want, (tid, s)


def test_the_blocks_philox_blocks_are_each_drawn_once():
    seen = np.zeros((32, 16), dtype=np.int64)
    for tid in range(256):
        col, blocks, _ = direct_map(tid)
        for q in blocks:
            assert 0 <= q < 16
            seen[col, q] += 1
    assert np.all(seen == 1)


def test_a_slot_is_the_row_the_product_fragment_expects():
    """fr_planes.h: lane (row of the operand = column l31, h) of fragment kg holds k = 16 kg + 8 (e / 4) + 4 h + e % 4; here kg = 4 R64 + f and
    k is the row of eps: the thread's block b, element r is row 4 (4 f + 2 b + h) + r of the 64-row block."""
    for tid in range(256):
        f, lane = tid >> 6, tid & 63
        h = lane >> 5
        _, blocks, _ = direct_map(tid)
        for e in range(8):
            assert 4 * blocks[e >> 2] + (e & 3) == 16 * f + 8 * (e // 4) + 4 * h + e % 4
