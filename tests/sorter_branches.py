"""Every text of tests/sorter_cases.py through the GPU builder on both engines: the suffix array (the samples of a
level-0 index ARE the suffix array; the 32-bit engine's kept one too) and the BWT against the oracle's.  Run in a child
process by tests/test_gpu_sorter_branches.py, which sets the library and the trace and reads the builder's trace from
stderr: a `CASE <name> <n> <engine>` line goes there before each build.
`python tests/sorter_branches.py small|threshold` prints "OK <builds>"."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import fm_index_amd as F              # noqa: E402
from oracle import fm_oracle as O     # noqa: E402
import sorter_cases as SC             # noqa: E402


def announce(case, engine):
    sys.stderr.write("CASE %s %d %s\n" % (case.name, case.n, engine))
    sys.stderr.flush()


def run(cases, engines):
    builds = 0
    for case in cases:
        t, n = case.text, case.n
        sa = O.suffix_array(t)
        if t.dtype == np.uint8:
            bwt = O.bwt(t, sa)
        else:                             # fm_index.rs:50-55, as the oracle's wide index builds it
            bwt = np.where(sa > 0, t[sa.astype(np.int64) - 1], 0).astype(t.dtype)
        cls = F.FMIndexMultiPiecesWithLocate if case.kind == "multi" else F.FMIndexWithLocate
        text = F.Text.with_max_character(t, case.max_character)
        for engine in engines:
            announce(case, engine)
            gi = cls(text, 0, force_wide=engine == "wide")
            sys.stderr.flush()
            assert gi.is_wide() == (engine == "wide")
            got = gi.export_sa_samples()
            assert len(got) == n and (got == sa).all(), ("sa", case.name, n, engine)
            assert (gi.export_bwt() == bwt).all(), ("bwt", case.name, n, engine)
            gi.close()
            builds += 1
            if engine == "32-bit":
                # a suffix array of its own allocation: small texts leave the pooled scratch (and only an index that
                # keeps its suffix array can run the builder's own check of it)
                announce(case, "keep-sa")
                gi = cls(text, 0, keep_sa=True)
                assert (gi.export_sa() == sa).all(), ("kept sa", case.name, n)
                assert gi.verify_sa() == 0, ("verify_sa", case.name, n, "keep-sa")
                gi.close()
                builds += 1
    print("OK", builds)
    return builds


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "small"
    if which == "small":
        run(SC.small_cases(), SC.ENGINES)
    elif which == "threshold":
        run(SC.threshold_cases(), ("32-bit",))
    else:
        sys.exit("usage: sorter_branches.py small|threshold")
