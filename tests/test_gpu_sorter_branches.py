"""Every exit of the prefix doubling of both GPU suffix sorters (suffix_sort, suffix_sort_wide in fmx_build.hip), on the
texts of tests/sorter_cases.py: the driver tests/sorter_branches.py compares the suffix array and the BWT with the
oracle's in a child process, and the builder's trace (measurement library, FMX_BUILD_TRACE) must show the exit and the
counts that the numpy model of tests/sorter_cases.py predicts -- so a case cannot pass through another branch."""
import os
import re
import subprocess
import sys

import pytest

import sorter_cases as SC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEASURE = os.path.join(ROOT, "fm_index_amd", "libfmx_measure.so")
# "[fmx build]   sort: tied       h=25          1.2 ms" / "[fmx build]   wide sort: text round h=6 ..."
TRACE_LINE = re.compile(r"^\[fmx build\]   (?:wide )?sort: (.+?)\s+h=(\d+)\s")


def drive(which, env_extra, n_builds):
    env = {k: v for k, v in os.environ.items() if k not in ("FMX_LIB", "FMX_BUILD_TRACE", "FMX_REFINE_MIN_N")}
    env.update(env_extra)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "sorter_branches.py"), which],
                         capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert "OK %d" % n_builds in out.stdout, out.stdout[-500:]
    return out.stderr


def sections(stderr):
    """{(name, n, engine): [(what, value)]} of the sorter's trace lines after each CASE line, "alloc" left out"""
    out, cur = {}, None
    for line in stderr.splitlines():
        if line.startswith("CASE "):
            _, name, n, engine = line.split()
            cur = out.setdefault((name, int(n), engine), [])
            assert not cur, "case announced twice: " + line
            continue
        m = TRACE_LINE.match(line)
        if m and cur is not None and m.group(1) != "alloc":
            cur.append((m.group(1), int(m.group(2))))
    return out


def branch_seen(events, n):
    """the exit a trace shows, by the lines alone"""
    kinds = [w for w, _ in events]
    if "tied" not in kinds:
        return 1 if kinds == ["round"] else None
    m = dict(events)["tied"]
    if 8 * m <= n:
        if "text round" not in kinds:
            return None
        return 2 if dict(events)["text round"] == 0 else 3
    last_full = max(h for w, h in events if w == "round")
    return 5 if 4 * last_full >= n else 4


def check_trace(events, case, engine):
    n = case.n
    p = SC.predict(case, "wide" if engine == "wide" else "32-bit")
    where = (case.name, n, engine, events)
    assert branch_seen(events, n) == p.branch == case.branch, where
    rest = [e for e in events if e[0] != "refine"]
    refines = len(events) - len(rest)
    assert events[len(rest):] == [e for e in events if e[0] == "refine"], where    # refine() comes last
    if p.branch == 1:
        assert events == [("round", p.k)], where
    elif p.branch in (2, 3):
        assert rest == [("round", p.k), ("tied", p.m), ("text round", p.m2)], where
        assert (refines == 0) if p.branch == 2 else (refines >= 1), where
    else:
        # full rounds: every count is the model's, none of them lets the text round in, and refine() takes over right
        # after the first count of n / 4 or less (the last full round of an all-equal text may leave nothing tied)
        want = [("round", p.k), ("tied", p.m)]
        for h, a in p.actives:
            want += [("active", a), ("round", 2 * h)]
        if p.actives[-1][0] == p.depth:
            want.pop()                                          # the hand-over: no further full round
        assert rest == want, where + (want,)
        assert all(8 * v > n for w, v in events if w == "tied"), where
        assert refines == p.refines, where
        if p.branch == 4:
            assert refines >= 1 and rest[-1][0] == "active", where
    return p


def test_branches_small():
    """both engines, refinement rounds forced on for every length (FMX_REFINE_MIN_N=0 in the measurement library)"""
    # no skip: the only deterministic coverage of the text round and of its hand-over to refine()
    assert os.path.exists(MEASURE), "fm_index_amd/libfmx_measure.so is missing: run `make -C fm_index_amd/csrc measure`"
    cases = SC.small_cases()
    err = drive("small", {"FMX_LIB": MEASURE, "FMX_BUILD_TRACE": "1", "FMX_REFINE_MIN_N": "0"}, 3 * len(cases))
    sec = sections(err)
    seen = {e: set() for e in SC.ENGINES}
    for case in cases:
        for engine in SC.ENGINES + ("keep-sa",):
            p = check_trace(sec[(case.name, case.n, engine)], case, engine)
            if engine in seen:
                seen[engine].add(p.branch)
    assert len(sec) == 3 * len(cases)
    assert seen == {e: {1, 2, 3, 4, 5} for e in SC.ENGINES}, seen


def test_threshold_with_trace():
    """kRefineMinN = 2^19 from both sides, 32-bit engine: at 2^19 - 1 nothing but full rounds, at 2^19 the predicted exit"""
    assert os.path.exists(MEASURE), "fm_index_amd/libfmx_measure.so is missing: run `make -C fm_index_amd/csrc measure`"
    cases = SC.threshold_cases()
    sec = sections(drive("threshold", {"FMX_LIB": MEASURE, "FMX_BUILD_TRACE": "1"}, 2 * len(cases)))
    for case in cases:
        for engine in ("32-bit", "keep-sa"):
            events = sec[(case.name, case.n, engine)]
            if case.n < 1 << 19:
                assert events and {w for w, _ in events} == {"round"}, (case.name, case.n, engine, events)
            else:
                check_trace(events, case, engine)
    assert {c.branch for c in cases} == {2, 3, 4}


def test_threshold_shipped():
    """the shipped library on the same texts (suffix array and BWT against the oracle's, in the driver): its builder is
    the traced one apart from the environment reads, so test_threshold_with_trace says which exit these builds take"""
    env = {"FMX_LIB": os.path.join(ROOT, "fm_index_amd", "libfmx.so")}
    err = drive("threshold", env, 2 * len(SC.threshold_cases()))
    assert not any(events for events in sections(err).values())      # (no trace in the shipped library)
