"""GPU tier of the point-decoder edge tests (cases: tests/decode_edges.py, whose expectations come from
the oracles alone; tests/test_decode_edges.py proves the builders on the CPU).

  Groth16   every alias twin (coordinate + p), every cofactor-torsion point as A, as C and as B, and the
            controls, in batches of 65 and 129 slots padded with valid proofs -- an alias twin in slot 0, a
            torsion case in slot n - 1 -- and alone (n = 1): zg_verify_each's statuses and left-hand sides,
            then both batch entries as tests/test_gpu_batch_edges.run_case compares them (statuses, the
            verdict, the bisection count, gt_out over exactly the slots of status 0 and 3), under the five
            MUTANT_SCHEDULES; once more in a child process on the library built with ZG_SUBGROUP_XX=1
  PGHR13    every alias twin of the seven G1 points and of b, alone and in one call past a wave, under every
            forced (B, K) launch shape of tests/test_gpu_pghr13_edges.py
  Jubjub    the alias key and the alias R through zg_redjubjub_verify, the alias cv / rk / epk through
            zg_prep_batch, an alias cv through zg_sapling_bvk, each at n = 1 and n = 65
  keys      an uncompressed verifying-key point with x + p or y + p through zg_vk_load_uncompressed"""
import os
import subprocess
import sys

import pytest

from tests import batch_edges as E, decode_edges as D, pghr13_edges as PE
from tests.conftest import ROOT
from tests.test_gpu_batch_edges import run_case
from tests.test_gpu_csum import _ctx_env

pytestmark = pytest.mark.gpu

XX_VARIANT = "xx"     # zebra_amd/libzg_xx.so: zg_decode.hip and zg_msm.hip with -DZG_SUBGROUP_XX=1 (build())


@pytest.fixture(scope="module", autouse=True)
def _device_alive():
    """one context open for the whole module, so the device's prepared keys outlive each test's own"""
    from zebra_amd import Context
    c = Context(device=0, max_batch=2)
    yield
    c.close()


def all_groth16_cases():
    """[(Case, name per slot | None)], the oracle's statuses held to the construction's"""
    out = []
    for case, who in [cw for n in D.BATCH_SIZES for cw in D.groth16_batches(n)] + D.single_lane_cases():
        assert case.statuses == D.expected_statuses(who), case.name
        out.append((case, [s and s.name for s in who]))
    return out


def each_check(c, case, names):
    """zg_verify_each: the restatement's status per slot and, where a proof decodes, its left-hand side"""
    want = case.statuses
    sts, gts = c.verify_each(case.proofs, case.kinds, case.inputs, case.nin)
    assert sts == want, (case.name, [(i, names[i], g, w) for i, (g, w) in enumerate(zip(sts, want)) if g != w])
    for i, g in enumerate(gts):
        assert g == (case._lhs[i] if want[i] in (0, 3) else None), (case.name, i, names[i])


def run_all(c, env, cases):
    for case, names in cases:
        each_check(c, case, names)
        run_case(c, env, case, partial=False, gt=True)


@pytest.mark.parametrize("env", E.MUTANT_SCHEDULES, ids=E.sched_id)
def test_groth16_alias_and_torsion(env):
    c = _ctx_env(env, E.MAX_BATCH)
    try:
        run_all(c, env, all_groth16_cases())
    finally:
        c.close()


def xx_child(path):
    """the body of test_groth16_alias_and_torsion_two_walk_subgroup_check, in a process of its own: the cases
    with the oracle's expectations as the parent formed them"""
    import pickle
    from zebra_amd import zg
    assert os.path.basename(zg.LIB_PATH) == "libzg_%s.so" % XX_VARIANT
    cases = []
    for name, proofs, kinds, inputs, r, nin, st, lhs, gt, names in pickle.load(open(path, "rb")):
        case = E.Case(name, proofs, kinds, inputs, r, nin, st, lhs)
        case._gt = gt
        cases.append((case, names))
    c = _ctx_env({}, E.MAX_BATCH)
    try:
        run_all(c, {}, cases)
    finally:
        c.close()
    print("xx ok %d" % len(cases))


def test_groth16_alias_and_torsion_two_walk_subgroup_check(tmp_path):
    """the same cases on the library built with ZG_SUBGROUP_XX=1 (G1's subgroup check as two walks of |x|,
    built and off by default). The library is chosen when zebra_amd.zg is imported, hence the child."""
    import pickle
    lib = os.path.join(ROOT, "zebra_amd", "libzg_%s.so" % XX_VARIANT)
    assert os.path.exists(lib), "zebra_amd/libzg_%s.so is not built (run __graft_entry__.build())" % XX_VARIANT
    cases = all_groth16_cases()
    path = str(tmp_path / "cases.pkl")
    pickle.dump([(c.name, c.proofs, c.kinds, c.inputs, c.r, c.nin, c.statuses, c._lhs, c.gt(), names)
                 for c, names in cases], open(path, "wb"))
    r = subprocess.run([sys.executable, "-c", "import sys; from tests.test_gpu_decode_edges import xx_child; "
                        "xx_child(sys.argv[1])", path],
                       cwd=ROOT, env=dict(os.environ, ZG_LIB_VARIANT=XX_VARIANT), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip().splitlines()[-1] == "xx ok %d" % len(cases)


# ------------------------------------------------------------------ PGHR13
@pytest.fixture(scope="module", params=PE.SHAPES, ids=PE.shape_id)
def shaped(request):
    from tests.test_gpu_pghr13_edges import _ctx_env as pg_ctx
    c = pg_ctx(request.param)
    yield request.param, c
    c.close()


def test_pghr13_alias_twins(shaped):
    """n = 1 (a G1 twin, a c1 twin, the q_big twin, a wrap twin) and every twin in one call past a wave:
    DECODE_INVALID for each twin, the valid proofs around them accepted on the one folded check"""
    from tests.test_gpu_pghr13_edges import _bk, _run
    env, ctx = shaped
    for case in D.pghr13_cases():
        _bk(ctx, env, case.n)
        assert not case.fails
        _run(ctx, case)


# ------------------------------------------------------------------ Jubjub
@pytest.fixture(scope="module")
def ctx():
    from zebra_amd import Context
    c = Context(device=0, max_batch=64)
    yield c
    c.close()


@pytest.mark.parametrize("n", [1, 65])
def test_redjubjub_alias_key_and_r(ctx, n):
    items = D.redjubjub_batch(n)
    got = ctx.redjubjub_verify([i.vk for i in items], [i.sig for i in items], [i.msg for i in items],
                               bytes(i.gen for i in items))
    assert got == [i.ok for i in items], [(i.name, g) for i, g in zip(items, got) if g != i.ok]


@pytest.mark.parametrize("n", [1, 65])
def test_prep_batch_alias_points(ctx, n):
    """zg_prep_batch: the oracle's rows for the small-y descriptions and the oracle's error code for each of
    cv / rk / epk as y + r; at n = 1 each job alone, at n = 65 all of them in one window, an alias job in
    the first and in the last slot"""
    from zebra_amd import zg as Z
    kind = {"spend": Z.PREP_KIND_SPEND, "output": Z.PREP_KIND_OUTPUT}
    code = {v: k for k, v in Z.PREP_ERRORS.items()}
    jobs = D.prep_jobs()
    good, bad = [j for j in jobs if j.want is None], [j for j in jobs if j.want]
    windows = [[j] for j in jobs] if n == 1 else [bad[:1] + [(good + bad)[i % len(jobs)] for i in range(n - 2)] + bad[-1:]]
    for w in windows:
        assert len(w) == n
        rows, codes = ctx.prep_batch(bytes(kind[j.kind] for j in w), b"".join(Z.prep_fields(kind[j.kind], *j.args) for j in w))
        for i, j in enumerate(w):
            assert codes[i] == (code[j.want] if j.want else 0), (i, j.name)
            if j.want is None:
                assert rows[288 * i:288 * i + 288] == Z.pack_inputs([D.prep_oracle_rows(j)]), (i, j.name)


@pytest.mark.parametrize("n", [1, 65])
def test_sapling_bvk_alias_cv(ctx, n):
    rows = D.bvk_rows()
    txs = [rows[1]] if n == 1 else [rows[1]] + [rows[i % 3] for i in range(n - 2)] + [rows[2]]
    got = ctx.sapling_bvk([(list(s), list(o), v) for s, o, v, _, _ in txs])
    assert got == [(st, bvk) for _, _, _, st, bvk in txs]
    assert got[0][0] == 1 and got[-1][0] == 1


# ------------------------------------------------------------------ uncompressed key points
def test_vk_load_uncompressed_refuses_a_coordinate_plus_p():
    """the error tests/test_vk_codec.py sees for a malformed key (ZG_E_VK), and the unchanged key loads"""
    from tests import cpulib
    from zebra_amd import Context
    from zebra_amd.zg import ZgError
    c = Context(device=0, max_batch=64, load_builtin=False)
    try:
        for name, kind, fields, ic in D.vk_alias_cases():
            with pytest.raises(ZgError) as e:
                c.vk_load_uncompressed(kind, *[fields[k] for k in D.VK_FIELDS], ic)
            assert e.value.code == -4, name
            good, good_ic = cpulib.vk_fields(kind)
            c.vk_load_uncompressed(kind, good[:96], good[96:192], good[192:384], good[384:576], good[576:672],
                                   good[672:864], good_ic)
            assert c.alpha_beta(kind) == D.B.f12_to_bytes(E.pvks()[kind].alpha_g1_beta_g2)
    finally:
        c.close()
