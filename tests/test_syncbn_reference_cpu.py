"""The two-rank SyncBatchNorm tests of tests/test_train_syncbn.py can fail: on exactly their inputs, every way a synced finalize
could be wrong without a one-rank test noticing (tests/syncref.py `played_ranks`) leaves the whole-batch float64 reference by at
least ten times the 2e-4 those tests allow, in the same measure — and the hand-written two-rank SyncBatchNorm itself, done right,
IS BatchNorm over the whole batch.  Float64 torch on the CPU only; no kernel is involved."""
import pytest

import syncref
from syncref import PWBN_SYNC_CASES, SEPBN_SYNC_CASES, STEM_SYNC_CASES, TOL, VARIANTS

_CASES = [("pwbn", c) for c in PWBN_SYNC_CASES] + [("stem", c) for c in STEM_SYNC_CASES] + [("sepbn", c) for c in SEPBN_SYNC_CASES]


def _setup(op, case):
    if op == "pwbn":
        inp = syncref.pwbn_sync_inputs(*case)
        return syncref.pwbn_sync_reference(inp, case[3]), lambda v: syncref.pwbn_played(inp, case[3], case[4], v), False
    if op == "stem":
        inp = syncref.stem_sync_inputs(*case)
        return syncref.stem_sync_reference(inp), lambda v: syncref.stem_played(inp, v), False
    inp = syncref.sepbn_sync_inputs(*case)
    return syncref.sepbn_sync_reference(inp), lambda v: syncref.sepbn_played(inp, v), case[5]


@pytest.mark.parametrize("op,case", _CASES, ids=[f"{op}-" + "x".join(str(int(v)) for v in c) for op, c in _CASES])
def test_every_wrong_sync_finalize_leaves_the_whole_batch_reference_by_ten_tolerances(op, case):
    ref, played, has_shift = _setup(op, case)
    right = syncref.compare(played("correct"), ref)
    assert max(right.values()) < 1e-9, right              # two ranks done right = the whole batch, to float64 rounding
    report = {}
    for variant in VARIANTS:
        if variant == "no_bias_shift" and not has_shift:  # (only a SepConv with biases has a shift to forget)
            continue
        errs = syncref.compare(played(variant), ref)
        worst = max(errs, key=errs.get)
        report[variant] = f"{worst}: {errs[worst]:.1e}"
        assert errs[worst] >= 10 * TOL, (variant, errs)
    print(report)
