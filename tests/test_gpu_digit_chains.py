"""GPU tier of the digit-resident lane R-chain (zg_lines.hip k_batch_lines_lane with ZG_LINES_FQD,
zg_lines.h lsd_double / lsd_add): forced with ZG_LINES_LANE = 1 and 2 (both register budgets) and
ZG_LINES_FCHAIN = 0 at n = 1, 63, 64, 65 and 129 proofs cut from tests/golden/batch64.json with its
r. Statuses and GT bytes against the fixture (its per-item lhs_gt), the 576-byte Miller partial
against the staged program's (ZG_LINES_LANE = 0). A B outside G2 in lanes 0, 63 and 64 in turn, and a
proof whose A does not decode next to an active one, must get the reference's status and leave
their neighbours' lines intact: the partial of the remaining proofs equals the staged program's.
(tests/test_digit_chains.py holds the step functions against the word form on the CPU.)"""
import pytest

from oracle import bls12_381 as B
from oracle import groth16 as G
from tests.conftest import load_golden
from tests.test_gpu_csum import _ctx_env
from tests.test_gpu_parity import fx_batch

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 129]
MAX_BATCH = 256


@pytest.fixture(scope="module")
def ctxs():
    cs = {m: _ctx_env({"ZG_LINES_LANE": m, "ZG_LINES_FCHAIN": 0}, MAX_BATCH) for m in (0, 1, 2)}
    yield cs
    for c in cs.values():
        c.close()


_ITEMS = None
_POW = {}


def items():
    global _ITEMS
    if _ITEMS is None:
        _ITEMS = load_golden("batch64.json")["items"]
    return _ITEMS


def cut(n, only_ok=False):
    """n items of the fixture, cyclically (with every corruption class it holds, or its valid ones only)"""
    src = [e for e in items() if e["status"] == 0] if only_ok else items()
    return [src[i % len(src)] for i in range(n)]


def item_pow(e):
    """lhs_gt ^ r of one fixture item, formed once"""
    k = (e["proof"], e["r"])
    if k not in _POW:
        _POW[k] = B.f12_pow(B.f12_from_bytes(bytes.fromhex(e["lhs_gt"])), G.batch_r(bytes.fromhex(e["r"])))
    return _POW[k]


def want_gt(its):
    acc = B.F12_ONE
    for e in its:
        if e["status"] in (0, 3):   # gt_out_def: the proofs that reach the pairing
            acc = B.f12_mul(acc, item_pow(e))
    return B.f12_to_bytes(acc)


def partial_of(c, proofs, kinds, inputs, nin, r, n):
    c.batch_begin(proofs, kinds, inputs, nin, r=r)
    part = c.batch_partial()
    sts = c.batch_finish(c.gt_check([part]), n)
    return part, sts


@pytest.mark.parametrize("lane", [1, 2])
@pytest.mark.parametrize("n", SIZES)
def test_lane_chain_on_batch64_cuts(ctxs, lane, n):
    its = cut(n)
    proofs, kinds, inputs, nin = fx_batch(its)
    r = b"".join(bytes.fromhex(e["r"]) for e in its)
    s0 = ctxs[lane].stats()
    sts, gt = ctxs[lane].verify_batch(proofs, kinds, inputs, nin, r=r, want_gt=True)
    assert sts == [e["status"] for e in its]
    assert gt == want_gt(its)
    part, sts = partial_of(ctxs[lane], proofs, kinds, inputs, nin, r, n)
    s1 = ctxs[lane].stats()
    assert s1["fused_launches"] == s0["fused_launches"]        # the split launches: the lane kernel ran
    assert sts == [e["status"] for e in its]
    ref, rsts = partial_of(ctxs[0], proofs, kinds, inputs, nin, r, n)
    assert rsts == sts
    assert part == ref


@pytest.mark.parametrize("lane", [1, 2])
@pytest.mark.parametrize("slot", [0, 63, 64])
def test_b_outside_g2_in_one_lane(ctxs, lane, slot):
    """the closing check fails that lane alone: DECODE_INVALID there, every other proof accepted, and
    the partial is the staged program's (the bad lane's lines are not in it, its neighbours' are)"""
    n = 129
    its = cut(n, only_ok=True)
    proofs, kinds, inputs, nin = fx_batch(its)
    r = b"".join(bytes.fromhex(e["r"]) for e in its)
    pr = bytearray(proofs)
    pr[192 * slot + 48:192 * slot + 144] = bytes.fromhex(load_golden("points.json")["g2_not_in_subgroup"])
    want = [1 if i == slot else 0 for i in range(n)]
    part, sts = partial_of(ctxs[lane], bytes(pr), kinds, inputs, nin, r, n)
    assert sts == want
    ref, rsts = partial_of(ctxs[0], bytes(pr), kinds, inputs, nin, r, n)
    assert rsts == want
    assert part == ref
    assert ctxs[lane].verify_batch(bytes(pr), kinds, inputs, nin, r=r)[0] == want


@pytest.mark.parametrize("lane", [1, 2])
def test_undecodable_a_next_to_active_proofs(ctxs, lane):
    """an A that does not decode (compression flag cleared) makes its lane inactive (identity lines);
    the lanes on both sides, across the wave boundary too, keep their lines"""
    n = 129
    its = cut(n, only_ok=True)
    proofs, kinds, inputs, nin = fx_batch(its)
    r = b"".join(bytes.fromhex(e["r"]) for e in its)
    pr = bytearray(proofs)
    bad = [1, 63, 64, 128]
    for i in bad:
        pr[192 * i] &= 0x7F
    want = [1 if i in bad else 0 for i in range(n)]
    part, sts = partial_of(ctxs[lane], bytes(pr), kinds, inputs, nin, r, n)
    assert sts == want
    ref, rsts = partial_of(ctxs[0], bytes(pr), kinds, inputs, nin, r, n)
    assert rsts == want
    assert part == ref
    # and the oracle's own partial for the first three slots (active, undecodable, active)
    if lane == 1:
        sp, sk, sx, sn = fx_batch(its[:3])
        sp = bytes(pr[:192 * 3])
        live = [(e["kind"], sp[192 * i:192 * i + 192], [int.from_bytes(bytes.fromhex(x), "little") for x in e["inputs"]],
                 G.batch_r(bytes.fromhex(e["r"]))) for i, e in enumerate(its[:3])]
        small, ssts = partial_of(ctxs[lane], sp, sk, sx, sn, r[:48], 3)
        assert ssts == [0, 1, 0]
        assert small == B.f12_to_bytes(G.batch_partial(_pvks(), live))


_PVKS = None


def _pvks():
    global _PVKS
    if _PVKS is None:
        import os
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        files = {0: "sapling-spend-verifying-key.json", 1: "sapling-output-verifying-key.json",
                 2: "sprout-groth16-key.json"}
        _PVKS = {k: G.prepare_verifying_key(G.load_vk_json(open(os.path.join(root, "zebra_amd", "res", f)).read()))
                 for k, f in files.items()}
    return _PVKS


# ---- decode's GLV products r_i A_i: the one-column form and the two-column form with its table in LDS
# (zg_decode.h k_decode_glv_lds, ZG_DEC_GLV_LDS), on the K4 grid layout (ZG_K4_MIN = 1, cglv = 0) and on
# the default layout of a lone small batch (cglv = 1: r_i C_i leaves, always one column), with r given
# explicitly: every pair of the edge scalars first, then seeded random rows.
GLV_EDGES = [0, 1, (1 << 64) - 1, 1 << 63, 0xAAAAAAAAAAAAAAAA, 0x5555555555555555]
GLV_ENVS = [{"ZG_K4_MIN": 1, "ZG_DEC_GLV_LDS": 0}, {"ZG_K4_MIN": 1, "ZG_DEC_GLV_LDS": 1}, {"ZG_DEC_GLV_LDS": 0},
            {"ZG_DEC_GLV_LDS": 1}]
_R16 = None
_GLV_PART = {}


def glv_r16(i):
    global _R16
    if _R16 is None:
        import random
        rng = random.Random(811)
        rows = [(a, b) for a in GLV_EDGES for b in GLV_EDGES] + \
            [(rng.getrandbits(64), rng.getrandbits(64)) for _ in range(max(SIZES))]
        _R16 = [a.to_bytes(8, "little") + b.to_bytes(8, "little") for a, b in rows]
    return _R16[i]


def glv_case(n):
    """n items of the fixture with the edge scalar rows: batch bytes, statuses, GT and the oracle's partial,
    formed once per size and shared by every environment"""
    if n not in _GLV_PART:
        its = cut(n)
        proofs, kinds, inputs, nin = fx_batch(its)
        r = b"".join(glv_r16(i) for i in range(n))
        acc = B.F12_ONE
        for i, e in enumerate(its):
            if e["status"] in (0, 3):
                k = (e["proof"], glv_r16(i))
                if k not in _POW:
                    _POW[k] = B.f12_pow(B.f12_from_bytes(bytes.fromhex(e["lhs_gt"])), G.batch_r(glv_r16(i)))
                acc = B.f12_mul(acc, _POW[k])
        live = [(e["kind"], bytes.fromhex(e["proof"]), [int.from_bytes(bytes.fromhex(x), "little") for x in e["inputs"]],
                 G.batch_r(glv_r16(i))) for i, e in enumerate(its)]
        part = B.f12_to_bytes(G.batch_partial(_pvks(), live))
        _GLV_PART[n] = (proofs, kinds, inputs, nin, r, [e["status"] for e in its], B.f12_to_bytes(acc), part)
    return _GLV_PART[n]


@pytest.fixture(scope="module")
def glv_ctxs():
    cs = [_ctx_env(env, MAX_BATCH) for env in GLV_ENVS]
    yield cs
    for c in cs:
        c.close()


@pytest.mark.parametrize("k", range(len(GLV_ENVS)), ids=["k4-onecol", "k4-lds", "cglv-onecol", "cglv-lds"])
@pytest.mark.parametrize("n", SIZES)
def test_glv_products_with_edge_scalars(glv_ctxs, k, n):
    proofs, kinds, inputs, nin, r, want, gt_want, part_want = glv_case(n)
    c = glv_ctxs[k]
    s0 = c.stats()
    sts, gt = c.verify_batch(proofs, kinds, inputs, nin, r=r, want_gt=True)
    s1 = c.stats()
    # the grid layout under test: K4 (cglv = 0) with ZG_K4_MIN = 1, the GLV C sums (cglv = 1) by default
    assert s1["glv_csum_batches"] - s0["glv_csum_batches"] == (0 if "ZG_K4_MIN" in GLV_ENVS[k] else 1)
    assert sts == want
    assert gt == gt_want
    part, sts = partial_of(c, proofs, kinds, inputs, nin, r, n)
    assert sts == want
    assert part == part_want
