"""TEST INFRASTRUCTURE ONLY: the word streams of the EXT_TRIGGER tests, shared by the CPU test (host form == checker) and the GPU
tests (device form == checker).  Words are built from the format descriptions in tests/ext_trigger_ref.py; nothing here decodes.

A case is (name, fmt, chunks, options): `chunks` a list of word arrays fed one after the other (the state carries), `options`
the decoder's (wait_for_time_base, legacy_halves)."""
import numpy as np

FMTS = (3, 2, 21)
DTYPE = {3: "<u2", 2: "<u4", 21: "<u8"}
N_IDS = {3: 16, 2: 32, 21: 32}
PER_BLOCK = 2048  # csrc/xmaps_evt.hpp: EVT_PER_BLOCK
BIG = PER_BLOCK * 257 + 5  # past one trip of 256 blocks in any per-block fold


def arr(fmt, words):
    return np.array([int(w) for w in words], dtype=np.uint64).astype(DTYPE[fmt])


def swap(words):
    w = np.asarray(words, dtype="<u8")
    return ((w << np.uint64(32)) | (w >> np.uint64(32))).astype("<u8")


# ---- single words ----
def trig(fmt, ident=0, value=1, low=0):
    if fmt == 3:
        return (0xA << 12) | (ident << 8) | value
    if fmt == 2:
        return (0xA << 28) | (low << 22) | (ident << 8) | value
    return (0xA << 60) | (low << 54) | (ident << 40) | (value << 32)


def th(fmt, v):
    return (0x8 << 12) | v if fmt == 3 else (0x8 << 28) | v if fmt == 2 else ((0x8 << 28) | v) << 32


def cd(fmt, x, y, p, low=0, mask=1):
    """one CD word: EVT 3.0 an ADDR_X (the row is whatever the stream set), EVT 2.0 a CD word, EVT 2.1 a word with `mask`"""
    if fmt == 3:
        return (0x2 << 12) | (p << 11) | x
    if fmt == 2:
        return (p << 28) | (low << 22) | (x << 11) | y
    return (((p << 28) | (low << 22) | (x << 11) | y) << 32) | mask


def tl3(v):
    return (0x6 << 12) | v


def y3(v):
    return v


def vbx3(x, p):
    return (0x3 << 12) | (p << 11) | x


def v12(mask):
    return (0x4 << 12) | mask


def v8(mask):
    return (0x5 << 12) | mask


# ---- random streams ----
def random_words(fmt, n, rng, trig_at=(), trig_rate=0.0, cd_rate=0.45):
    """n words of every type the format has, payloads random; EXT_TRIGGER words at `trig_at` and at a random `trig_rate` of places"""
    if fmt == 3:
        kinds = np.array([0x0, 0x2, 0x3, 0x4, 0x5, 0x6, 0x8, 0xE, 0x7])
        p = np.array([0.08, cd_rate, 0.06, 0.05, 0.03, 0.15, 0.03, 0.02, 0.01])
        k = rng.choice(kinds, n, p=p / p.sum())
        w = (k.astype(np.uint64) << np.uint64(12)) | rng.integers(0, 1 << 12, n).astype(np.uint64)
        # TIME_HIGH mostly creeps upwards (random values would wrap at every other word; some still do)
        hi = np.nonzero(k == 0x8)[0]
        vals = (np.cumsum(rng.integers(0, 3, len(hi))) + 0xFF0) & 0xFFF
        jump = rng.random(len(hi)) < 0.05
        vals = np.where(jump, rng.integers(0, 1 << 12, len(hi)), vals)
        w[hi] = (np.uint64(0x8) << np.uint64(12)) | vals.astype(np.uint64)
    else:
        kinds = np.array([0x0, 0x1, 0x8, 0xE, 0xF, 0x3])
        p = np.array([cd_rate / 2, cd_rate / 2, 0.08, 0.02, 0.01, 0.01])
        k = rng.choice(kinds, n, p=p / p.sum())
        top = (k.astype(np.uint64) << np.uint64(28)) | rng.integers(0, 1 << 28, n).astype(np.uint64)
        hi = np.nonzero(k == 0x8)[0]
        vals = (np.cumsum(rng.integers(0, 3, len(hi))) + 0x0FFFFFF0) & 0x0FFFFFFF
        jump = rng.random(len(hi)) < 0.05
        vals = np.where(jump, rng.integers(0, 1 << 28, len(hi)), vals)
        top[hi] = (np.uint64(0x8) << np.uint64(28)) | vals.astype(np.uint64)
        if fmt == 2:
            w = top
        else:
            mask = (rng.integers(0, 1 << 32, n) & rng.integers(0, 1 << 32, n) & rng.integers(0, 1 << 32, n)).astype(np.uint64)
            w = (top << np.uint64(32)) | mask
    at = np.array(sorted(set(int(i) for i in trig_at) | set(np.nonzero(rng.random(n) < trig_rate)[0].tolist())), dtype=np.int64)
    for i in at:
        w[i] = trig(fmt, int(rng.integers(0, N_IDS[fmt])), int(rng.integers(0, 2)), int(rng.integers(0, 64)))
    return w.astype(DTYPE[fmt])


def is_trigger(fmt, words):
    w = np.asarray(words, dtype=DTYPE[fmt]).astype(np.uint64)
    return (w >> np.uint64({3: 12, 2: 28, 21: 60}[fmt])) == 0xA


# ---- the cases ----
def sized_cases(fmt):
    """chunk sizes: one word; the block size and its neighbours; past one trip of 256 blocks -- a trigger as the first and the last
    word of the chunk and of a block, two and three adjacent ones"""
    out = []
    rng = np.random.default_rng(100 + fmt)
    out.append(("one trigger word", fmt, [arr(fmt, [trig(fmt, 3, 1, 9)])], {}))
    out.append(("one event word after a time base", fmt, [arr(fmt, [th(fmt, 5)]), arr(fmt, [cd(fmt, 7, 2, 1)]), arr(fmt, [trig(fmt, 1, 0, 2)])], {}))
    for n in (PER_BLOCK - 1, PER_BLOCK, PER_BLOCK + 1):
        out.append((f"{n} words", fmt, [random_words(fmt, n, rng, trig_at=(0, n - 1, 700, 701, 1200, 1201, 1202), trig_rate=0.002)], {}))
    at = (0, BIG - 1, PER_BLOCK - 1, PER_BLOCK, 2 * PER_BLOCK - 1, 256 * PER_BLOCK - 1, 256 * PER_BLOCK, 256 * PER_BLOCK + 1,
          257 * PER_BLOCK, 5000, 5001, 9000, 9001, 9002)
    out.append(("past 256 blocks", fmt, [random_words(fmt, BIG, rng, trig_at=at, trig_rate=0.0005, cd_rate=0.2)], {}))
    return out


def small_cases(fmt):
    out = []
    rng = np.random.default_rng(200 + fmt)
    out.append(("triggers only", fmt, [arr(fmt, [trig(fmt, i % N_IDS[fmt], i & 1, i % 64) for i in range(300)])], {}))
    out.append(("no trigger", fmt, [random_words(fmt, 3000, rng)], {}))
    ids = [th(fmt, 77)]
    for i in range(N_IDS[fmt]):
        for v in (0, 1):
            ids += [cd(fmt, i, 3, 1, 5), trig(fmt, i, v, (i + v) % 64)]
    out.append(("every id, both values", fmt, [arr(fmt, ids)], {}))
    pre = [trig(fmt, 1, 1, 3), cd(fmt, 9, 1, 1, 4), trig(fmt, 2, 0, 5), th(fmt, 3), trig(fmt, 3, 1, 6), cd(fmt, 10, 1, 0, 7), trig(fmt, 4, 0, 8)]
    for wait in (False, True):
        out.append((f"in front of the first time base, wait={wait}", fmt, [arr(fmt, pre)], {"wait_for_time_base": wait}))
        out.append((f"in front of the first time base, chunked, wait={wait}", fmt, [arr(fmt, pre[:2]), arr(fmt, pre[2:3]), arr(fmt, pre[3:])],
                    {"wait_for_time_base": wait}))
        w = random_words(fmt, 2 * PER_BLOCK + 100, rng, trig_rate=0.01)
        first = PER_BLOCK + 37  # the first time base lies in the second block: the first block emits nothing when waiting
        hi_kind = 0x8
        shift = {3: 12, 2: 28, 21: 60}[fmt]
        kinds = (w.astype(np.uint64) >> np.uint64(shift))
        w[:first][kinds[:first] == hi_kind] = arr(fmt, [cd(fmt, 1, 1, 1)])[0]
        w[first] = arr(fmt, [th(fmt, 9)])[0]
        out.append((f"first time base in the second block, wait={wait}", fmt, [w], {"wait_for_time_base": wait}))
    if fmt == 3:
        out.append(("trigger between VECT_BASE_X and VECT_12", 3,
                    [arr(3, [th(3, 5), tl3(7), y3(3), vbx3(100, 1), trig(3, 2, 1), v12(0b101), trig(3, 3, 0), v8(0b11), cd(3, 4, 0, 0)])], {}))
        out.append(("trigger behind a TIME_HIGH that changed without a TIME_LOW", 3,
                    [arr(3, [th(3, 5), tl3(9), cd(3, 1, 0, 1), trig(3, 0, 1), th(3, 6), trig(3, 1, 1), cd(3, 2, 0, 1), th(3, 6), trig(3, 2, 1),
                             tl3(4), trig(3, 3, 1)])], {}))
        out.append(("trigger behind a 24-bit wrap", 3,
                    [arr(3, [th(3, 0xFFF), tl3(1), cd(3, 1, 0, 1), trig(3, 0, 1), th(3, 1), trig(3, 1, 1), tl3(2), cd(3, 2, 0, 1), trig(3, 2, 0)])], {}))
    else:
        out.append(("trigger behind a TIME_HIGH loop", fmt,
                    [arr(fmt, [th(fmt, 0x0FFFFFF0), cd(fmt, 1, 1, 1, 3), trig(fmt, 0, 1, 4), th(fmt, 5), trig(fmt, 1, 1, 6), cd(fmt, 2, 1, 0, 7)])], {}))
    if fmt == 21:
        full = [th(21, 11)]
        for i in range(40):
            full += [cd(21, 32 * (i % 8), i, i & 1, i % 64, 0xFFFFFFFF), trig(21, i % 32, i & 1, (i * 3) % 64)]
        out.append(("triggers between words of 32 events", 21, [arr(21, full)], {}))
        out.append(("legacy halves", 21, [swap(arr(21, full))], {"legacy_halves": True}))
        out.append(("legacy halves, random", 21, [swap(random_words(21, 5000, rng, trig_rate=0.01))], {"legacy_halves": True}))
    return out


def split_cases(fmt):
    """about 6000 words decoded whole and split at every position of a 64-word window around a trigger"""
    rng = np.random.default_rng(300 + fmt)
    w = random_words(fmt, 6000, rng, trig_at=(3000,), trig_rate=0.003)
    out = [("6000 words whole", fmt, [w], {})]
    for s in range(3000 - 32, 3000 + 32):
        out.append((f"6000 words split at {s}", fmt, [w[:s], w[s:]], {}))
    return out


def all_cases(fmt):
    return sized_cases(fmt) + small_cases(fmt) + split_cases(fmt)
