"""The coherent queues' per-wave cursors (csrc/rtw_wavefront.hip wf_push_bucketed): a host model of one wave
drives the device's slot arithmetic (rtw_wavefront.h wf_cursor_*, through rtw_debug_push_cursor).

The model keeps what the wave keeps in LDS -- per bucket the open block `blk` and the next free slot `cur`,
cur == blk + 64 meaning no open block -- and the stripe counter the fresh blocks come from.  A push: every
pushing lane adds 1 to its bucket's cursor (in any order: the LDS unit serialises the lanes of one bucket),
reads blk, and either has its slot or is lane j of the bucket's overflow; the lanes with j = 0 open the fresh
blocks (one add on the stripe counter for all of them, in lane order), store blk and rebase cur; the other
overflow lanes read blk back and take fresh + j.

Checked: a bucket's slots are exactly the consecutive slots of its blocks (no duplicate, no gap before cur),
one block is taken per overflow, and the dead range at close is [cur, blk + 64)."""
import numpy as np
import pytest

BUCKETS = 16
NO_OVER = 0xFFFFFFFF


def cursor(rtw, blk, old, fresh):
    blk, old, fresh = (np.ascontiguousarray(x, np.uint32) for x in (blk, old, fresh))
    n = blk.size
    slot, over, rebase = (np.zeros(n, np.uint32) for _ in range(3))
    rc = rtw.lib().rtw_debug_push_cursor(n, blk.ctypes.data, old.ctypes.data, fresh.ctypes.data, slot.ctypes.data,
                                         over.ctypes.data, rebase.ctypes.data)
    assert rc == 0
    return slot, over, rebase


class Wave:
    """One wave's cursors and its stripe counter; `base` is the stripe's first slot (s * stripe_cap)."""

    def __init__(self, rtw, rng, base=0, fills=None):
        self.rtw, self.rng, self.base = rtw, rng, base
        self.len = 0                                # the stripe counter (slots handed out, relative to base)
        self.blocks = [[] for _ in range(BUCKETS)]  # per bucket: the blocks it has held, in order
        self.given = [[] for _ in range(BUCKETS)]   # per bucket: the slots handed to lanes, in cursor order
        self.prefill = [0] * BUCKETS                # slots of the first block that were used before the model starts
        self.fresh_blocks = 0
        self.overflows = 0
        self.virtual = fills is None
        if fills is None:  # the kernel's start (wf_open_cursors): no bucket has an open block, i.e. every bucket
            fills = [64] * BUCKETS  # a full "block" at slot 0 that is nobody's (none of its slots is ever given)
            self.blk = np.zeros(BUCKETS, np.uint32)
        else:              # bucket b starts with an open block of its own holding fills[b] slots (64: full)
            self.blk = np.uint32(base) + np.arange(BUCKETS, dtype=np.uint32) * np.uint32(64)
            self.len = 64 * BUCKETS
        self.cur = self.blk + np.asarray(fills, np.uint32)
        for b in range(BUCKETS):
            self.blocks[b].append(int(self.blk[b]))
            self.prefill[b] = int(fills[b])

    def push(self, keys):
        """keys[l]: lane l's bucket, -1 = the lane does not push.  Returns the lanes' slots (-1: none)."""
        keys = np.asarray(keys)
        lanes = np.flatnonzero(keys >= 0)
        old = np.zeros(64, np.uint32)
        for l in self.rng.permutation(lanes):  # the atomics of one push in any order
            old[l] = self.cur[keys[l]]
            self.cur[keys[l]] += np.uint32(1)
        blk = self.blk[keys[lanes]]
        _, over, _ = cursor(self.rtw, blk, old[lanes], np.zeros(lanes.size, np.uint32))
        openers = lanes[over == 0]  # lane order: the ballot's rank
        assert len(set(keys[openers])) == openers.size, "two lanes open a block for one bucket"
        over_keys = set(keys[lanes[over != NO_OVER]])
        assert over_keys == set(keys[openers]), "an overflowing bucket without its j = 0 lane"
        b0 = self.base + self.len
        self.len += 64 * openers.size
        self.fresh_blocks += openers.size
        self.overflows += len(over_keys)
        old_blk = self.blk.copy()
        for r, l in enumerate(openers):
            f = np.uint32(b0 + 64 * r)
            _, _, rebase = cursor(self.rtw, [old_blk[keys[l]]], [old[l]], [f])
            self.blk[keys[l]] = f
            self.cur[keys[l]] = (int(self.cur[keys[l]]) + int(rebase[0])) & 0xFFFFFFFF  # (wraps, as on the device)
            self.blocks[keys[l]].append(int(f))
        # every lane: its slot from the block it read first and, for an overflow lane, the block read back
        slot, _, _ = cursor(self.rtw, blk, old[lanes], self.blk[keys[lanes]])
        out = np.full(64, -1, np.int64)
        out[lanes] = slot
        for b in range(BUCKETS):
            mine = lanes[keys[lanes] == b]
            self.given[b] += [int(out[l]) for l in mine[np.argsort(old[mine])]]
        return out

    def check(self):
        seen = set()
        for b in range(BUCKETS):
            # the consecutive slots of the bucket's blocks, the first block from its prefill on
            want = [blk + k for i, blk in enumerate(self.blocks[b]) for k in range(self.prefill[b] if i == 0 else 0, 64)]
            n = len(self.given[b])
            assert sorted(self.given[b]) == want[:n], f"bucket {b}: slots are not its blocks' consecutive slots"
            assert not seen & set(self.given[b]), "a slot handed out twice"
            seen |= set(self.given[b])
            # close (wf_close_blocks): the dead slots are [cur, blk + 64), all that is left of the open block
            cur, blk = int(self.cur[b]), int(self.blk[b])
            assert blk == self.blocks[b][-1] and blk <= cur <= blk + 64
            assert list(range(cur, blk + 64)) == want[n:], f"bucket {b}: dead range"
            # one block per overflow: exactly the blocks the bucket's slots need
            assert len(self.blocks[b]) == max(1, (self.prefill[b] + n + 63) // 64), f"bucket {b}: blocks"
        assert self.fresh_blocks == self.overflows == sum(len(x) - 1 for x in self.blocks)
        own = 0 if self.virtual else BUCKETS
        assert self.len == 64 * (own + self.fresh_blocks)  # the stripe holds these blocks and no more


def prefilled(rtw, rng, fills, base=0):
    return Wave(rtw, rng, base, fills)


def random_keys(rng, n_lanes, n_buckets):
    keys = np.full(64, -1)
    lanes = rng.choice(64, n_lanes, replace=False)
    keys[lanes] = rng.integers(0, n_buckets, n_lanes)
    return keys


def test_arithmetic(rtw):
    """wf_cursor_over / _slot / _rebase at the block's ends."""
    blk = np.array([0, 0, 0, 640, 640, 640, 640, 0xFFFFFF00], np.uint32)
    old = np.array([0, 63, 64, 640, 703, 704, 767, 0xFFFFFF40], np.uint32)
    fresh = np.full(8, 1280, np.uint32)
    slot, over, rebase = cursor(rtw, blk, old, fresh)
    assert list(over) == [NO_OVER, NO_OVER, 0, NO_OVER, NO_OVER, 0, 63, 0]
    assert list(slot) == [0, 63, 1280, 640, 703, 1280, 1343, 1280]
    assert list(rebase[:4]) == [1280 - 64, 1280 - 64, 1280 - 64, 1280 - 704]
    # the opener's rebase moves a cursor that counted k lanes past the old block to fresh + k
    assert (704 + 5 + int(rebase[3])) & 0xFFFFFFFF == 1280 + 5


@pytest.mark.parametrize("fill", range(65))
def test_every_starting_fill(rtw, fill):
    """Every bucket starts with `fill` slots of its block used; random pushes of 1..64 lanes."""
    rng = np.random.default_rng(fill)
    w = prefilled(rtw, rng, [fill] * BUCKETS, base=4096 * (fill % 3))
    for _ in range(12):
        w.push(random_keys(rng, int(rng.integers(1, 65)), int(rng.choice([1, 2, 4, 16]))))
    w.check()


@pytest.mark.parametrize("room", [0, 1, 63])
def test_whole_wave_in_one_bucket(rtw, room):
    """All 64 lanes share one key and its block has room for 0, 1 or 63 of them."""
    rng = np.random.default_rng(100 + room)
    fills = [64 - room] * BUCKETS
    w = prefilled(rtw, rng, fills)
    keys = np.full(64, 5)
    out = w.push(keys)
    first = int(w.blocks[5][0])
    assert sorted(out)[:room] == list(range(first + 64 - room, first + 64))
    assert len(w.blocks[5]) == 2 and sorted(out)[room:] == list(range(w.blocks[5][1], w.blocks[5][1] + 64 - room))
    assert int(w.cur[5]) == w.blocks[5][1] + 64 - room
    w.check()
    for _ in range(3):  # and again: every push of 64 lanes overflows once
        w.push(keys)
    w.check()
    assert len(w.blocks[5]) == 5


def test_from_the_kernels_start(rtw):
    """wf_open_cursors' state (blk 0, cur 64 for every bucket): the first push of a bucket opens its first
    block, mixed lane counts and key sets after that."""
    rng = np.random.default_rng(7)
    for base in (0, 64 * 1000):
        w = Wave(rtw, rng, base)
        for k in range(40):
            n = 64 if k % 7 == 0 else int(rng.integers(1, 65))
            w.push(random_keys(rng, n, int(rng.choice([1, 3, 16]))))
        w.check()
        assert all(s >= base for g in w.given for s in g)
