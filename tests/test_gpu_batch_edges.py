"""GPU tier: zg_verify_batch and zg_batch_begin / zg_batch_partial / zg_batch_finish at ragged sizes
(n < npad), under every launch schedule, on edge inputs -- the cases of tests/batch_edges.py, whose
expectations come from the oracle alone (tests/test_batch_edges.py proves the builders on the CPU).

  1  ragged sweep: n in {1, 2, 3, 5, 31, 33, 65, 129, 257}, clean and corrupted at slot 0, an interior slot
     and slot n - 1, under every schedule; the launch path zg_stats reports is the one the library's own
     clamps (run_pipeline, zebra_amd/csrc/zg.hip) select at that size, the fallback where they exclude it
  2  kind mixes: Sprout / output / spend only and each pair, n in {3, 33}
  3  the 9 real proofs and the 71 builtin-key mutants in ONE batch (n = 80, five rotations)
  4  degenerate sums: equal and opposite r_i C_i meeting in the C-sum tree and in one K4 bucket (the
     H == 0 branches of zg_fqd.h / zg_curve.h on the device), nothing live, extreme scalar and input rows
  5  API corners: a clean shard finished with batch_ok = 0, n = 0

Statuses, gt_out and the 576-byte partial are compared bit for bit.
Reference: verify_proof and its callers' precedence, verification/src/sapling.rs:157-167,
verification/src/sprout.rs:73-77."""
import pytest

from tests import batch_edges as E
from tests.test_gpu_csum import _ctx_env

pytestmark = pytest.mark.gpu

STAT_OF_PATH = {"fused": "fused_launches", "quads": "quad_fchain_launches", "lineprod": "line_product_batches",
                "affine": "affine_line_batches"}


@pytest.fixture(scope="module", autouse=True)
def _device_alive():
    """one context open for the whole module, so the device's prepared keys outlive each test's own
    context (zg_destroy of the last context frees them)"""
    from zebra_amd import Context
    c = Context(device=0, max_batch=2)
    yield
    c.close()


def _path_check(env, case, s0, s1):
    """the stats' account of one batch against the clamps' restatement -> the path's name"""
    want = E.expected_path(env, case.npad)
    got = {k: s1[v] - s0[v] for k, v in STAT_OF_PATH.items()}
    got["k4"] = 1 - (s1["glv_csum_batches"] - s0["glv_csum_batches"])
    assert s1["batches"] - s0["batches"] == 1 and s1["fused_wait_failures"] == 0
    assert got == {k: int(v) for k, v in want.items()}, (E.sched_id(env), case.name, got, want)
    if want["k4"] and case.live:   # (nothing live: a B still owing its G2 check is counted, then recomputed)
        assert s1["k4_entries"] > 0, case.name
    if not want["k4"]:
        assert s1["k4_entries"] == 0, case.name
    return E.path_name(want)


def run_case(c, env, case, partial=True, gt=True):
    """both entries on one case: begin / partial / verdict / finish, then verify_batch"""
    want_st = case.statuses
    clean = 3 not in want_st
    s0 = c.stats()
    c.batch_begin(case.proofs, case.kinds, case.inputs, case.nin, r=case.r)
    part = c.batch_partial()
    verdict = c.gt_check([part])
    sts = c.batch_finish(verdict, case.n)
    s1 = c.stats()
    path = _path_check(env, case, s0, s1)
    assert verdict == clean, case.name
    assert sts == want_st, case.name
    assert s1["bisections"] - s0["bisections"] == (0 if clean else 1), case.name
    if partial:
        assert part == case.partial(affine=E.expected_path(env, case.npad)["affine"]), case.name
    sts, out = c.verify_batch(case.proofs, case.kinds, case.inputs, case.nin, r=case.r, want_gt=gt)
    s2 = c.stats()
    assert _path_check(env, case, s1, s2) == path
    assert sts == want_st, case.name
    assert s2["bisections"] - s1["bisections"] == (0 if clean else 1), case.name
    if gt:
        assert out == case.gt(), case.name
    return path


def _limits(case):
    return {"partial": case.n <= E.PARTIAL_MAX and 3 not in case.statuses and 1 not in case.statuses,
            "gt": case.n <= E.GT_MAX}


@pytest.mark.parametrize("env", E.SCHEDULES, ids=E.sched_id)
def test_ragged_sweep(env):
    """every size of the sweep, clean and corrupted, plus the always-corrupted batches of one and two
    proofs: oracle statuses, verdict, reject set, the partial up to 33 proofs and gt_out up to 129"""
    cases = []
    for n in E.SIZES:
        cases.append(E.ragged_clean(n))
        if n >= 3:
            cases.append(E.ragged_corrupt(n))
    cases += E.minimal_bad()
    c = _ctx_env(env, E.MAX_BATCH)
    try:
        paths = [(case.n, run_case(c, env, case, **_limits(case))) for case in cases]
    finally:
        c.close()
    print("paths %s: %s" % (E.sched_id(env), " ".join("%d:%s" % p for p in sorted(set(paths)))))
    # the sweep reaches the intended path wherever the clamps allow it, and the fallback elsewhere
    want = {E.npad_of(n): E.path_name(E.expected_path(env, E.npad_of(n))) for n in E.SIZES}
    assert {E.npad_of(n): p for n, p in paths} == want


@pytest.mark.parametrize("env", E.SCHEDULES, ids=E.sched_id)
def test_kind_mixes(env):
    """one key or two keys absent from the batch (empty sums), n = 3 and 33, clean and corrupted"""
    c = _ctx_env(env, E.MAX_BATCH)
    try:
        for case in E.all_mix_cases():
            run_case(c, env, case, **_limits(case))
    finally:
        c.close()


@pytest.mark.parametrize("env", E.MUTANT_SCHEDULES, ids=E.sched_id)
def test_all_mutants_in_one_batch(env):
    """n = 80 with every corruption class of the fixture, MALFORMED_VK and INPUT_NONCANONICAL slots
    among them: the fixture's statuses, and gt_out over exactly its status-0 and status-3 items; five
    rotations put each class once first and once last (next to the padding)"""
    base = E.mutant_batch()
    c = _ctx_env(env, E.MAX_BATCH)
    try:
        for case in [base] + [base.rotated(k) for k in E.MUTANT_ROTATIONS]:
            run_case(c, env, case, partial=False, gt=True)
    finally:
        c.close()


@pytest.mark.parametrize("env", E.SCHEDULES, ids=E.sched_id)
def test_degenerate_batches(env):
    """D1 - D7 on the C-sum tree (ZG_K4_MIN = 2^30) and on K4's buckets (ZG_K4_MIN = 1): statuses,
    gt_out and the partial's bytes"""
    for k4_min in (1, 1 << 30):
        e = dict(env, ZG_K4_MIN=k4_min)
        c = _ctx_env(e, E.MAX_BATCH)
        try:
            for case in E.degenerate_cases():
                run_case(c, e, case)
        finally:
            c.close()


@pytest.mark.parametrize("env", [{}, {"ZG_LINES_FCHAIN": 0, "ZG_FCHAIN_QUADS": 1, "ZG_LINE_GROUP": 32}], ids=E.sched_id)
def test_clean_shard_finished_as_failed(env):
    """another rank spoiled the combined verdict: zg_batch_finish(batch_ok = 0) on a clean shard of 33
    bisects once (the root passes its own check) and returns all OK"""
    case = E.ragged_clean(33)
    c = _ctx_env(env, E.MAX_BATCH)
    try:
        c.batch_begin(case.proofs, case.kinds, case.inputs, r=case.r)
        part = c.batch_partial()
        assert part == case.partial() and c.gt_check([part])
        before = c.stats()["bisections"]
        assert c.batch_finish(False, case.n) == [0] * case.n
        assert c.stats()["bisections"] == before + 1
    finally:
        c.close()


def test_empty_batch():
    """n = 0 (include/zg.h): zg_verify_batch returns ZG_OK, writes no status and gt_out = 1; the split
    form gives the empty partial (1), which passes zg_gt_check, and finishes with either verdict"""
    case = E.empty_batch()
    c = _ctx_env({}, E.MAX_BATCH)
    try:
        sts, gt = c.verify_batch(b"", b"", b"", r=b"", want_gt=True)
        assert sts == [] and gt == case.gt()
        sts, gt = c.verify_batch(b"", b"", b"", want_gt=True)
        assert sts == [] and gt == case.gt()
        for ok in (True, False):
            c.batch_begin(b"", b"", b"")
            part = c.batch_partial()
            assert part == case.partial() and c.gt_check([part])
            assert c.batch_finish(ok, 0) == []
        # the context is as usable as before
        one = E.ragged_clean(1)
        assert c.verify_batch(one.proofs, one.kinds, one.inputs, r=one.r, want_gt=True) == ([0], one.gt())
    finally:
        c.close()
