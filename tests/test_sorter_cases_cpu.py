"""The texts of tests/sorter_cases.py take the exits of the prefix doubling they are meant to take -- by the numpy model
of the counts the GPU sorters branch on -- and the oracle's suffix array of exactly these texts is the naive one.
tests/test_gpu_sorter_branches.py then holds the builder's trace to the same counts."""
import numpy as np
import pytest

import sorter_cases as SC
from oracle import fm_oracle as O

SMALL = SC.small_cases()
IDS = ["%s-%d" % (c.name, c.n) for c in SMALL]


def check_branch(case, engine):
    n = case.n
    p = SC.predict(case, engine)
    assert p.branch == case.branch, (case.name, n, engine, p)
    if p.branch == 1:
        assert p.m == 0
    elif p.branch == 2:
        assert 0 < 8 * p.m <= n and p.m2 == 0
    elif p.branch == 3:
        assert 0 < 8 * p.m <= n and p.m2 > 0
    else:
        assert 8 * p.m > n
        assert all(4 * a > n for _, a in p.actives[:-1])
        if p.branch == 4:
            # an `active` count of at most n / 4 that is not 0, early: refine() takes over on the compacted list
            assert p.actives[-1][0] == p.depth and 0 < 4 * p.actives[-1][1] <= n
            assert 4 * p.depth < n and p.refines >= 1
        else:
            assert 4 * p.depth >= n
    return p


@pytest.mark.parametrize("case", SMALL, ids=IDS)
def test_small_case_takes_its_branch(case):
    for engine in SC.ENGINES:
        check_branch(case, engine)


def test_small_cases_cover_every_branch_at_every_size():
    for n in SC.SMALL_SIZES:
        assert {c.branch for c in SMALL if c.n == n} == {1, 2, 3, 4, 5}, n
    # only the plants of 2k + 5 symbols and more cannot keep 8 m <= n at n = 257
    assert {name for name in SC.GENERATORS for n in SC.SMALL_SIZES if SC.make(name, n) is None} == \
        {"long-copies", "copy-of-the-tail"}


def test_tail_copy_and_zero_runs_reach_the_padding():
    """copy-of-the-tail: tied suffixes whose text key at depth k is packed from past the end; zero-runs: the terminator's
    suffix is tied with interior runs of zeros, at depth k and at depth 2k (so the tied group holds sorted position 0)"""
    for n in SC.SMALL_SIZES[1:]:
        c = SC.make("copy-of-the-tail", n)
        k = SC.key_symbols(c.max_character, "32-bit")
        assert (c.text[n // 2:n // 2 + 2 * k + 5] == c.text[n - 1 - (2 * k + 5):n - 1]).all()
        assert c.text[n // 2 + 2 * k + 5] != 0
    for n in SC.SMALL_SIZES + SC.THRESHOLD_SIZES:
        c = SC.make("zero-runs", n)
        for engine in SC.ENGINES:
            k = SC.key_symbols(c.max_character, engine)
            nonzero = np.concatenate([[0], np.cumsum(np.concatenate([c.text, np.zeros(2 * k, dtype=np.uint8)]) != 0)])
            for depth in (k, 2 * k):
                zero_heads = np.flatnonzero(nonzero[depth:depth + n] == nonzero[:n])   # `depth` zeros from there on
                assert n - 1 in zero_heads and len(zero_heads) > 1, (n, engine, depth)


@pytest.mark.parametrize("case", [c for c in SMALL if c.n <= 4099], ids=[i for i, c in zip(IDS, SMALL) if c.n <= 4099])
def test_oracle_suffix_array_is_the_naive_one(case):
    assert (O.suffix_array(case.text) == O.suffix_array(case.text, naive=True)).all()


@pytest.mark.parametrize("name", SC.THRESHOLD_CASES)
def test_threshold_case_takes_its_branch(name):
    """the same generator on both sides of kRefineMinN = 2^19 (the model is the one of enabled refinement rounds: what
    the shipped library does at 2^19, and would do at 2^19 - 1 if the threshold were lower)"""
    for n in SC.THRESHOLD_SIZES:
        check_branch(SC.make(name, n), "32-bit")
