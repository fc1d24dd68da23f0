"""NumPy's ziggurat normal sampler on an explicit list of raw 64-bit values, in plain Python: the reference for
the device-side continuation of the NumPy stream (csrc/obe_rng.hip) on streams NumPy itself cannot be fed.

* ``classify(raw, i)``    one draw "as if a normal started at position i": (value, length, margin), with the
                          kernel's two limits (length 0 = ran off the buffer, or more than 32 raw values).
* ``table(raw)``          the same for every position (what zig_classify_kernel writes).
* ``chain(tab, first)``   the real parse from ``first``: start positions, values, end of every draw.
* ``anchors(tab, first)`` positions no jump can skip (what zig_starts_kernel looks for).
* ``Builder``             hand-built draws of every length from the bit fields of a raw value, and the crafted
                          streams the tests run (``mixed_stream``, ``ones_stream``), with the conditions they must
                          meet (``check_stream``).

Bit fields of a raw value r (random_standard_normal): idx = bits 0-7, sign = bit 8, rabs = bits 9-60; the
same value as a uniform is bits 11-63 (next_double).  ``margin`` is the smallest relative distance from a tie
over the accept/reject decisions of a draw: |lhs - rhs| / max(lhs, rhs) in a wedge, |2 yy - xx^2| / max(2 yy, xx^2)
in the tail (inf for a draw that decides nothing); a stream whose margins are all >= 1e-6 is parsed the same way
by any exp/log1p that is accurate to a few ulp.
"""
import math
import os
import random

import numpy as np

ZIG_R = 3.6541528853610087963519472518
ZIG_INV_R = 0.27366123732975827203338247596
MAX_LEN = 32                         # kMaxLen: longest draw handled on the device
TILE = 2048                          # kStartTile = kFlagTile: positions per workgroup of the start flags / compaction
END_GUARD = 2 * MAX_LEN              # obe_ziggurat_check: the n-th normal must end this far before the buffer's end
MASK52 = (1 << 52) - 1
U53 = 1.0 / 9007199254740992.0
MIN_MARGIN = 1e-6

_HERE = os.path.dirname(os.path.abspath(__file__))
_Z = np.load(os.path.join(os.path.dirname(_HERE), "optbayesexpt_amd", "data", "ziggurat_tables.npz"))
KI_ARR, WI_ARR, FI_ARR = _Z["ki"].astype(np.uint64), _Z["wi"].astype(np.float64), _Z["fi"].astype(np.float64)
KI, WI, FI = [int(k) for k in KI_ARR], WI_ARR.tolist(), FI_ARR.tolist()

BODY, TAIL = 0, 1                    # kind of an accepted draw: rectangle / wedge value, or tail value (log1p)


def _rel(a, b):
    m = max(a, b)
    return abs(a - b) / m if m > 0.0 else 0.0


def classify_kind(raw, i, n=None):
    """(value, length, margin, kind) of the draw that starts at raw[i] in a buffer of ``n`` values (default: all)."""
    n = len(raw) if n is None else n
    left = n - i
    used, x, margin = 0, 0.0, math.inf
    while True:
        if used >= left or used >= MAX_LEN:
            return x, 0, margin, BODY
        r = int(raw[i + used])
        used += 1
        idx, sign, rabs = r & 0xff, (r >> 8) & 1, (r >> 9) & MASK52
        x = rabs * WI[idx]
        if sign:
            x = -x
        if rabs < KI[idx]:
            return x, used, margin, BODY
        if idx == 0:
            while True:
                if used + 1 >= left or used + 2 > MAX_LEN:
                    return x, 0, margin, BODY
                xx = -ZIG_INV_R * math.log1p(-((int(raw[i + used]) >> 11) * U53))
                yy = -math.log1p(-((int(raw[i + used + 1]) >> 11) * U53))
                used += 2
                margin = min(margin, _rel(yy + yy, xx * xx))
                if yy + yy > xx * xx:
                    return (-(ZIG_R + xx) if (rabs >> 8) & 1 else ZIG_R + xx), used, margin, TAIL
        else:
            if used >= left:
                return x, 0, margin, BODY
            u = (int(raw[i + used]) >> 11) * U53
            used += 1
            lhs, rhs = (FI[idx - 1] - FI[idx]) * u + FI[idx], math.exp(-0.5 * x * x)
            margin = min(margin, _rel(lhs, rhs))
            if lhs < rhs:
                return x, used, margin, BODY


def classify(raw, i, n=None):
    """(value, length, margin) for a normal starting at position ``i``; length 0 = off the buffer or > 32 values."""
    return classify_kind(raw, i, n)[:3]


class Table:
    """Per-position classification of a buffer: val, len (uint8), margin, kind."""

    def __init__(self, raw, n=None):
        raw = np.ascontiguousarray(raw, dtype=np.uint64)
        n = raw.size if n is None else int(n)
        raw = raw[:n]
        idx = (raw & np.uint64(0xff)).astype(np.intp)
        rabs = (raw >> np.uint64(9)) & np.uint64(MASK52)
        x = rabs.astype(np.float64) * WI_ARR[idx]
        x = np.where((raw >> np.uint64(8)) & np.uint64(1), -x, x)
        slow = np.flatnonzero(rabs >= KI_ARR[idx])
        self.n = n
        self.val = x
        self.len = np.ones(n, dtype=np.uint8)
        self.margin = np.full(n, np.inf)
        self.kind = np.zeros(n, dtype=np.uint8)
        rawl = raw.tolist()
        for i in slow.tolist():                      # the rest end inside their rectangle: one value, no decision
            self.val[i], self.len[i], self.margin[i], self.kind[i] = classify_kind(rawl, i, n)
        self.n_slow = slow.size


def table(raw, n=None):
    return Table(raw, n)


def chain(tab, first=0, n_normals=None):
    """The parse from ``first``: (start positions, values, kinds, ends) of the normals found — all of them up to a
    position that cannot be classified, or the first ``n_normals``.  ends[-1] - first is what they consumed."""
    lens = tab.len.tolist()
    starts, p, n = [], int(first), tab.n
    while p < n and lens[p] and (n_normals is None or len(starts) < n_normals):
        starts.append(p)
        p += lens[p]
    starts = np.asarray(starts, dtype=np.int64)
    return starts, tab.val[starts], tab.kind[starts], starts + tab.len[starts]


def anchors(tab, first=0):
    """Boolean per position: a (>= first) is an anchor iff no q in [max(first, a - 32), a) has q + len[q] > a.
    Lengths are at most 32, so "the 32 predecessors" and "every predecessor" are the same set of conditions."""
    reach = np.arange(tab.n, dtype=np.int64) + tab.len
    out = np.zeros(tab.n, dtype=bool)
    out[first] = True
    if tab.n > first + 1:
        out[first + 1:] = np.maximum.accumulate(reach[first:-1]) <= np.arange(first + 1, tab.n)
    return out


def anchors_by_definition(tab, first=0):
    """anchors() spelled out position by position over the window of 32 predecessors (test of the shortcut)."""
    lens = tab.len.tolist()
    out = np.zeros(tab.n, dtype=bool)
    for a in range(first, tab.n):
        out[a] = all(q + lens[q] <= a for q in range(max(first, a - MAX_LEN), a))
    return out


def nearest_anchor(tab, first=0):
    """For every position p >= first the nearest anchor at or before it (-1 below ``first``)."""
    a = anchors(tab, first)
    pos = np.where(a, np.arange(tab.n), -1)
    return np.maximum.accumulate(pos)


def check_stream(raw, n_raw=None, first=0):
    """The conditions every crafted stream handed to the device must meet; returns (table, chain).
    * every position has decision margin >= 1e-6;
    * every true start more than 64 positions before the end has length 1 .. 32;
    * consecutive anchors are at most 32 apart: every position, the last 64 included (the kernel flags those too
      and counts them in `found`), has its nearest anchor at most 31 positions back (the kernel's design contract)."""
    tab = table(raw, n_raw)
    worst = int(np.argmin(tab.margin))
    assert tab.margin[worst] >= MIN_MARGIN, (worst, tab.margin[worst])
    ch = chain(tab, first)
    starts = ch[0]
    inner = starts[starts < tab.n - END_GUARD]
    assert np.all((tab.len[inner] >= 1) & (tab.len[inner] <= MAX_LEN))
    # the chain reaches the guard zone: no true start before it is unclassifiable
    assert starts.size and ch[3][-1] >= tab.n - END_GUARD, (first, tab.n, ch[3][-1] if starts.size else None)
    near = nearest_anchor(tab, first)
    p = np.arange(first, tab.n)       # (to the very end: the kernel flags the last 64 positions too, and `found` counts them)
    back = p - near[p]
    assert back.max() <= MAX_LEN - 1, (int(p[np.argmax(back)]), int(back.max()))
    return tab, ch


def normals_within(ch, n_raw, first=0):
    """How many normals of the chain end at least 64 positions before the end: the most a caller may ask for."""
    return int(np.sum(ch[3] <= n_raw - END_GUARD))


# ------------------------------------------------------------------ draw gadgets
def first_word(idx, sign, rabs, top3):
    """A raw value by its fields as the first value of a draw; bits 61-63 (``top3``) only matter when the value is
    read as a uniform: u = top3 / 8 + rabs / 2^55."""
    assert 0 <= idx < 256 and 0 <= rabs <= MASK52 and 0 <= top3 < 8
    return idx | (sign << 8) | (rabs << 9) | (top3 << 61)


def uniform_word(u53, low11):
    """A raw value by its fields as a uniform: u = u53 / 2^53; bits 0-10 (``low11``) only matter when the value is
    read as the first value of a draw: idx = bits 0-7, sign = bit 8, and the two lowest bits of rabs."""
    assert 0 <= u53 < (1 << 53) and 0 <= low11 < (1 << 11)
    return (u53 << 11) | low11


_RECT_IDX = [0] + list(range(2, 256))                                # ki[1] = 0: layer 1 has no rectangle
_WIDE_IDX = [i for i in range(256) if KI[i] >= (9 << 52) // 10 + 4]  # rabs < 0.9 * 2^52 is inside the rectangle


class Builder:
    """Raw streams from draw gadgets.  Every value is built so that it also parses comfortably when read in its
    other role (a uniform as the first value of a draw, a first value as a uniform): check_stream() asserts it."""

    def __init__(self, seed):
        self.rnd = random.Random(seed)
        self.words = []
        self.draws = []               # (start, length, description) of the gadgets as built

    def __len__(self):
        return len(self.words)

    def _low11(self, idxs):
        return self.rnd.choice(idxs) | (self.rnd.getrandbits(3) << 8)

    def _top3(self):
        return self.rnd.randint(2, 6)                # as a uniform: 0.25 <= u < 0.875

    # -- single values
    def _rect(self):
        idx = self.rnd.choice(_RECT_IDX)
        return first_word(idx, self.rnd.getrandbits(1), self.rnd.randrange(KI[idx]), self._top3())

    def _wedge_reject(self):
        """rabs = 2^52 - 1: x at the outer edge of the layer, exp(-x^2/2) ~ fi[idx]; u ~ 1: lhs ~ fi[idx - 1]."""
        idx = self.rnd.randint(1, 255)
        return [first_word(idx, self.rnd.getrandbits(1), MASK52, self._top3()),
                uniform_word((1 << 53) - 1, self._low11(range(1, 256)))]

    def _wedge_accept(self):
        """rabs = ki[idx]: x at the inner edge, exp(-x^2/2) ~ fi[idx - 1]; u ~ 0: lhs ~ fi[idx]."""
        idx = self.rnd.randint(1, 255)
        return [first_word(idx, self.rnd.getrandbits(1), KI[idx], self._top3()),
                uniform_word(self.rnd.getrandbits(20), self._low11(_RECT_IDX))]

    def _tail(self, k):
        """idx = 0 beyond the base strip's rectangle, k rejected pairs (u ~ 1: xx ~ 10; u = 0.25: 2 yy = 0.58), then
        an accepted pair (u <= 0.49: xx <= 0.19; u >= 0.625: 2 yy >= 1.96)."""
        w = [first_word(0, self.rnd.getrandbits(1), self.rnd.randrange(KI[0], 1 << 52), self._top3())]
        for _ in range(k):
            w.append(uniform_word((1 << 53) - 1, self._low11(range(1, 256))))
            w.append(uniform_word(1 << 51, self._low11(_RECT_IDX)))
        mid = lambda: self.rnd.randrange((9 << 50) // 10)          # noqa: E731  (as a first value: inside a wide rectangle)
        w.append(uniform_word((self.rnd.randint(1, 3) << 50) | mid(), self._low11(_WIDE_IDX)))
        w.append(uniform_word((self.rnd.randint(5, 6) << 50) | mid(), self._low11(_WIDE_IDX)))
        return w

    # -- draws
    def fill(self, count=1):
        for _ in range(count):
            self.draws.append((len(self.words), 1, "rect"))
            self.words.append(self._rect())

    def fill_to(self, pos):
        assert pos >= len(self.words)
        self.fill(pos - len(self.words))

    def draw(self, rejects, ending, pairs=0):
        """``rejects`` wedge rejections, then ``ending``: "rect" (1 value), "wedge" (2) or "tail" (3 + 2 pairs).
        A draw of wedge rejections that ends in a rectangle is followed by one filler value: the parse that starts
        on its second value runs one value past its end, and must not run on into the next long draw."""
        w = []
        for _ in range(rejects):
            w += self._wedge_reject()
        w += {"rect": lambda: [self._rect()], "wedge": self._wedge_accept, "tail": lambda: self._tail(pairs)}[ending]()
        assert len(w) <= MAX_LEN
        self.draws.append((len(self.words), len(w), f"{rejects}r+{ending}{pairs if ending == 'tail' else ''}"))
        self.words += w
        if rejects and ending == "rect":
            self.fill(1)
        return len(w)

    def draw_of_length(self, length, tail=False):
        """A draw of exactly ``length`` values: wedge rejections and a rectangle (odd) or a wedge accept (even);
        ``tail``: a tail draw (odd lengths from 3)."""
        if tail:
            assert length >= 3 and length % 2 == 1
            return self.draw(0, "tail", (length - 3) // 2)
        return self.draw((length - 1) // 2, "rect") if length % 2 else self.draw(length // 2 - 1, "wedge")

    def array(self):
        return np.array(self.words, dtype=np.uint64)


def gadget_lengths():
    """One stream per draw length 1 .. 32 (and the tail draws of length 3 .. 31): [(length, raw)], the draw first,
    then filler.  For the test that the gadgets give every chain length."""
    out = []
    for length in range(1, MAX_LEN + 1):
        for tail in ((False, True) if length % 2 and length >= 3 else (False,)):
            b = Builder(1000 + length)
            b.draw_of_length(length, tail)
            b.fill(3 * MAX_LEN)
            out.append((length, tail, b.array()))
    return out


MIXED_N_RAW = 3 * TILE + 5
MIXED_VARIANTS = 8


def straddle_plan(variant):
    """(boundary, start, length, tail) of the long draws a mixed stream places across its first two tile
    boundaries, the start at a different residue modulo 8 in every variant: the longest draw there is (32 values:
    15 wedge rejections and a wedge accept) from T - 31 .. T - 24, and a tail draw of 31 from T - 30 .. T - 23.
    (The third boundary is 5 values from the end of the stream: nothing that crosses it can be asked for.)"""
    plan = []
    for b in range(2):
        T = (b + 1) * TILE
        length, tail = ((32, False), (31, True))[b]
        back = (31, 30)[b] - (variant + 3 * b) % 8
        plan.append((T, T - back, length, tail))
    return plan


def mixed_stream(variant=0):
    """3 * 2048 + 5 raw values: draws of every length in shuffled order with short runs of one-value draws
    between them, the long draws of straddle_plan() across the first two tile boundaries, one-value draws
    across the third and 5 values of a fourth tile."""
    b = Builder(4200 + variant)
    forced = straddle_plan(variant)
    while True:
        specs = [(length, False) for length in range(1, MAX_LEN + 1)] + [(length, True) for length in range(3, 32, 2)]
        specs += [("combo", b.rnd.randint(1, 6), b.rnd.randint(0, 7)) for _ in range(6)]
        b.rnd.shuffle(specs)
        for spec in specs:
            need = 2 * MAX_LEN + 2           # (room for any gadget, its filler and a run of one-value draws)
            if forced and len(b) + need > forced[0][1]:
                T, start, length, tail = forced.pop(0)
                b.fill_to(start)
                b.draw_of_length(length, tail)
                assert start < T < start + length
            if len(b) + need > MIXED_N_RAW - 3 * MAX_LEN and not forced:
                b.fill_to(MIXED_N_RAW)
                return b
            if spec[0] == "combo":
                b.draw(spec[1], "tail", spec[2])     # wedge rejections, then a tail draw: 2 j + 3 + 2 k <= 29
            else:
                b.draw_of_length(*spec)
            b.fill(b.rnd.choice((0, 0, 1, 2, 5)))


def ones_stream(n_raw, seed=7):
    """Every draw one value long."""
    b = Builder(seed)
    b.fill(n_raw)
    return b


# ------------------------------------------------------------------ the crafted cases of the GPU tests
ONES_N_RAW = 2 * TILE + 300
MIXED_SIZES = (TILE - 1, TILE, TILE + 1, MIXED_N_RAW)
DEFERRED_N_RAW = 2 * TILE + 500          # a third tile of 500 values: room for an n-th normal in the last tile

_STREAMS = {}


def stream(kind, variant):
    """The full raw stream of a family ("mixed": mixed_stream(variant); "ones": ones_stream, seed = variant)."""
    if (kind, variant) not in _STREAMS:
        b = mixed_stream(variant) if kind == "mixed" else ones_stream(ONES_N_RAW, seed=variant)
        _STREAMS[kind, variant] = b.array()
    return _STREAMS[kind, variant]


_CASES = {}


def case(kind, variant, n_raw, first=0):
    """(raw[:n_raw], table, chain from ``first``) of a crafted stream — handed out only after check_stream() has
    passed on exactly this buffer and this ``first``: nothing out of contract reaches the device."""
    key = (kind, variant, n_raw, first)
    if key not in _CASES:
        raw = stream(kind, variant)[:n_raw].copy()
        assert raw.size == n_raw
        _CASES[key] = (raw,) + check_stream(raw, n_raw, first)
    return _CASES[key]


OFFSET_NAMES = ("true_start_aligned", "true_start_not_multiple_of_8", "second_value_of_a_long_draw",
                "third_value_of_a_long_draw", "second_tile_true_start", "second_tile_inside_a_long_draw",
                "65_before_the_end")


def mixed_offsets(variant=0):
    """Where the mixed stream is entered with ``offset`` > 0: name -> offset."""
    _, tab, (starts, _, _, _) = case("mixed", variant, MIXED_N_RAW)
    lens = tab.len
    long_ = [int(s) for s in starts if lens[s] >= 24]
    pick = lambda cond: next(int(s) for s in starts if cond(int(s)))          # noqa: E731
    return {
        "true_start_aligned": pick(lambda s: s >= 100 and s % 8 == 0),
        "true_start_not_multiple_of_8": pick(lambda s: s >= 300 and s % 8 == 5),
        "second_value_of_a_long_draw": long_[0] + 1,           # the u ~ 1 of a rejection, read as a first value
        "third_value_of_a_long_draw": long_[1] + 2,            # the rest of the same draw, shorter
        "second_tile_true_start": pick(lambda s: s >= TILE + 600 and s % 8 == 3),
        "second_tile_inside_a_long_draw": next(s for s in long_ if s >= TILE + 2 * MAX_LEN) + 1,
        "65_before_the_end": MIXED_N_RAW - END_GUARD - 1,
    }


def crafted_cases():
    """Every (kind, variant, n_raw, first) the GPU tests upload."""
    out = [("mixed", v, n_raw, 0) for v in range(MIXED_VARIANTS) for n_raw in MIXED_SIZES]
    out += [("mixed", 0, MIXED_N_RAW, off) for off in mixed_offsets(0).values()]
    out += [("ones", 7, ONES_N_RAW, off) for off in (0, 5, TILE + 3)]
    out += [("mixed", 3, DEFERRED_N_RAW, 0)]
    return out


# ------------------------------------------------------------------ real PCG64 streams
FALLBACK_N, FALLBACK_D, FALLBACK_SEED = 70_001, 5, 99


def numpy_consumption(seed, n_uniform, n_normal):
    """Raw values that ``n_normal`` standard normals consume after ``n_uniform`` uniforms of default_rng(seed)."""
    raw = np.random.default_rng(seed).bit_generator.random_raw(n_uniform + n_normal + n_normal // 8 + 4096)
    ends = chain(table(raw[n_uniform:]), 0, n_normal)[3]
    assert ends.size == n_normal
    return int(ends[-1])
