"""The ziggurat oracle (tests/_ziggurat_oracle.py) without a GPU: it reproduces numpy.random.Generator bit for
bit, and the crafted raw streams the GPU tests feed to obe_ziggurat_normal meet — as conditions computed from
the oracle alone — the contract of the device code and the coverage they were built for."""
import numpy as np
import pytest
from numpy.testing import assert_array_equal

import _ziggurat_oracle as zo


@pytest.mark.parametrize("seed", [3, 11, 2024])
def test_oracle_reproduces_numpy(seed):
    """200 000 normals: the same values, the same number of raw values consumed (the generator state after
    advance(consumed) is numpy's) — what lets the oracle stand in for numpy on streams numpy cannot be fed."""
    n = 200_000
    raw = np.random.default_rng(seed).bit_generator.random_raw(n + n // 24 + 4096)
    ref = np.random.default_rng(seed)
    want = ref.standard_normal(n)
    tab = zo.table(raw)
    starts, vals, kinds, ends = zo.chain(tab, 0, n)
    assert starts.size == n
    assert_array_equal(vals, want)
    assert_array_equal(kinds == zo.TAIL, np.abs(want) > zo.ZIG_R)
    moved = np.random.default_rng(seed)
    moved.bit_generator.advance(int(ends[-1]))
    assert moved.bit_generator.state == ref.bit_generator.state
    # the table's vectorised rectangle path is classify(), position by position
    rawl = raw.tolist()
    for i in list(range(0, 3000)) + list(range(raw.size - 40, raw.size)):
        v, length, margin = zo.classify(rawl, i)
        assert (v, length) == (tab.val[i], tab.len[i]) or (length == 0 and tab.len[i] == 0), i
        assert margin == tab.margin[i]


def test_gadgets_give_every_chain_length():
    seen = set()
    for length, tail, raw in zo.gadget_lengths():
        value, got, margin = zo.classify(raw.tolist(), 0)
        assert got == length and margin >= zo.MIN_MARGIN
        assert (abs(value) > zo.ZIG_R) == tail
        tab, (starts, _, _, _) = zo.check_stream(raw)
        assert starts[1] == length
        seen.add((length, tail))
    assert {length for length, _ in seen} == set(range(1, 33))
    assert (31, True) in seen and (32, False) in seen


def test_limits_of_one_draw():
    """The kernel's two limits: a draw that needs a 33rd value, or a value past the end of the buffer, has length 0."""
    b = zo.Builder(1)
    for _ in range(16):
        b.words += b._wedge_reject()
    b.words += b._wedge_accept()
    raw = b.words
    assert zo.classify(raw, 0)[1] == 0                      # 34 values
    assert zo.classify(raw, 2)[1] == 32
    assert zo.classify(raw, 2, n=33)[1] == 0                # the 32nd value would be raw[33]
    assert zo.classify(raw, 2, n=34)[1] == 32
    b = zo.Builder(2)
    b.draw(0, "tail", 14)
    assert zo.classify(b.words, 0)[1] == 31
    assert zo.classify(b.words, 0, n=30)[1] == 0
    b = zo.Builder(3)
    b.words += b._tail(15)                                  # a 16th pair: 33 values
    b.fill(40)
    assert zo.classify(b.words, 0)[1] == 0


def test_anchor_shortcut_is_the_definition():
    for key in (("mixed", 0, zo.MIXED_N_RAW, 0), ("mixed", 5, zo.TILE + 1, 0),
                ("mixed", 0, zo.MIXED_N_RAW, zo.mixed_offsets(0)["second_value_of_a_long_draw"])):
        _, tab, _ = zo.case(*key)
        assert_array_equal(zo.anchors(tab, key[3]), zo.anchors_by_definition(tab, key[3]))


def test_offset_names_are_the_offsets():
    assert tuple(zo.mixed_offsets(0)) == zo.OFFSET_NAMES


def test_crafted_streams_meet_the_contract():
    keys = zo.crafted_cases()
    assert len(keys) == len(set(keys)) == 43
    for key in keys:
        _one_crafted_stream(key)


def _one_crafted_stream(key):
    """Margins >= 1e-6 at every position, true starts of length 1 .. 32, an anchor at least every 32 positions:
    asserted by check_stream() inside case(), for the buffer length and the first position the GPU test uses."""
    raw, tab, (starts, vals, kinds, ends) = zo.case(*key)
    assert raw.size == key[2] and starts[0] == key[3]
    assert tab.margin.min() >= zo.MIN_MARGIN
    assert zo.normals_within((starts, vals, kinds, ends), key[2]) >= 1


def test_offsets_enter_the_stream_where_they_say():
    _, tab, (starts, _, _, ends) = zo.case("mixed", 0, zo.MIXED_N_RAW)
    off = zo.mixed_offsets(0)
    true = set(starts.tolist())
    assert off["true_start_aligned"] in true and off["true_start_aligned"] % 8 == 0
    assert off["true_start_not_multiple_of_8"] in true and off["true_start_not_multiple_of_8"] % 8 != 0
    assert off["second_tile_true_start"] in true and off["second_tile_true_start"] > zo.TILE + 2 * zo.MAX_LEN
    for name in ("second_value_of_a_long_draw", "third_value_of_a_long_draw", "second_tile_inside_a_long_draw"):
        o = off[name]
        assert o not in true
        s = int(starts[np.searchsorted(starts, o) - 1])
        assert tab.len[s] >= 24 and s < o < s + int(tab.len[s])
        # the parse from there is another one for a while: it is re-chained, not cut out of the parse from 0
        mine = zo.case("mixed", 0, zo.MIXED_N_RAW, o)[2][0]
        assert mine[0] == o and len(set(mine[:3].tolist()) - true) >= 1
    assert off["second_tile_inside_a_long_draw"] > zo.TILE + 2 * zo.MAX_LEN
    assert any(o % 8 for o in off.values())
    assert off["65_before_the_end"] == zo.MIXED_N_RAW - 65


def test_crafted_streams_cover_what_they_were_built_for():
    lengths, residues, deepest, tail_pairs = set(), set(), False, 0
    for v in range(zo.MIXED_VARIANTS):
        _, tab, (starts, vals, kinds, ends) = zo.case("mixed", v, zo.MIXED_N_RAW)
        lens = tab.len[starts]
        ok = ends <= zo.MIXED_N_RAW - zo.END_GUARD           # (only draws a caller can ask for count)
        lengths |= set(lens[ok].tolist())
        near = zo.nearest_anchor(tab)
        for T in (zo.TILE, 2 * zo.TILE):
            across = ok & (starts < T) & (ends > T) & (lens >= 24)
            residues |= {(T, int(s) % 8) for s in starts[across]}
            deepest |= bool(near[T] == T - (zo.MAX_LEN - 1))
        tails = ok & (kinds == zo.TAIL)
        tail_pairs = max(tail_pairs, int(((lens[tails] - 3) // 2).max()))     # (an upper bound unless the draw is pure tail)
        # 32 = 15 wedge rejections + a wedge accept; 31 also as a pure tail draw (1 + 15 pairs)
        assert np.any(lens[ok] == 32) and np.any(tails & (lens == 31))
    assert lengths == set(range(1, 33))
    assert {r for T, r in residues if T == zo.TILE} == set(range(8))
    assert {r for T, r in residues if T == 2 * zo.TILE} == set(range(8))
    assert deepest
    # at least one tail draw with >= 3 rejected pairs, counted on the gadget as built (no wedge rejections in front)
    pure = [d for v in range(zo.MIXED_VARIANTS) for d in zo.mixed_stream(v).draws if d[2].startswith("0r+tail")]
    assert max(int(d[2][len("0r+tail"):]) for d in pure) >= 3 and tail_pairs >= 3


def test_resample_fallback_seed_outruns_the_smallest_buffer():
    """The condition of the GPU test of resample()'s fallback: for n = 70 001 particles, d = 5 and
    default_rng(99), numpy's n d normals consume more than n d + 4096 - 64 raw values, so the smallest buffer
    obe_resample_begin accepts is too short."""
    n, d, seed = zo.FALLBACK_N, zo.FALLBACK_D, zo.FALLBACK_SEED
    consumed = zo.numpy_consumption(seed, n, n * d)
    assert consumed > n * d + 4096 - zo.END_GUARD
    ref = np.random.default_rng(seed)
    ref.random(n)
    ref.standard_normal(n * d)
    moved = np.random.default_rng(seed)
    moved.bit_generator.advance(n + consumed)
    assert moved.bit_generator.state == ref.bit_generator.state
