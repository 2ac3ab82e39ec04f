"""GPU tier of decode's G1 point chains (zg_decode.h k_decode_points over zg_fqd.h: the point formulas
closed by one sum of two products, in the GLV products and the subgroup checks; with ZG_SUBGROUP_XX
the subgroup check as two walks of |x| with its re-added point in LDS): batches of n = 1, 63, 64, 65
and 129 proofs cut from tests/golden/batch64.json with its r, under both decode grid layouts -- K4
(ZG_K4_MIN = 1, cglv = 0) and the GLV C sums of a lone small batch (cglv = 1: C's leaves r_i C_i run
the same GLV chain). Statuses and GT bytes against the fixture, the 576-byte Miller partial against
the oracle's.

Then the A, and separately the C, of the proof in lane 0, 63 and 64 in turn is replaced by a curve
point outside G1 -- the point of order 3 (0, 2) and the fixture's g1_not_in_subgroup: the oracle gives
the status, and the partial must be the oracle's for the remaining proofs (the neighbours, across the
wave boundary too, are untouched). (tests/test_g1_digit_chains.py holds the formulas on the CPU.)"""
import pytest

from oracle import bls12_381 as B
from oracle import groth16 as G
from tests.conftest import load_golden
from tests.test_gpu_csum import _ctx_env
from tests.test_gpu_digit_chains import _pvks, cut, partial_of, want_gt
from tests.test_gpu_parity import fx_batch

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 129]
MAX_BATCH = 256
ENVS = [{"ZG_K4_MIN": 1}, {}]
IDS = ["k4", "cglv"]
BAD_N = 65          # lanes 0, 63 and 64: both sides of the wave boundary


@pytest.fixture(scope="module")
def ctxs():
    cs = [_ctx_env(env, MAX_BATCH) for env in ENVS]
    yield cs
    for c in cs:
        c.close()


def live_of(its, proofs):
    return [(e["kind"], proofs[192 * i:192 * i + 192], [int.from_bytes(bytes.fromhex(x), "little") for x in e["inputs"]],
             G.batch_r(bytes.fromhex(e["r"]))) for i, e in enumerate(its)]


_CASE = {}


def case(n):
    """n items of the fixture with its r: batch bytes, statuses, GT and the oracle's partial, formed once
    per size and shared by both layouts"""
    if n not in _CASE:
        its = cut(n)
        proofs, kinds, inputs, nin = fx_batch(its)
        r = b"".join(bytes.fromhex(e["r"]) for e in its)
        part = B.f12_to_bytes(G.batch_partial(_pvks(), live_of(its, proofs)))
        _CASE[n] = (proofs, kinds, inputs, nin, r, [e["status"] for e in its], want_gt(its), part)
    return _CASE[n]


@pytest.mark.parametrize("k", range(len(ENVS)), ids=IDS)
@pytest.mark.parametrize("n", SIZES)
def test_decode_chains_on_batch64_cuts(ctxs, k, n):
    proofs, kinds, inputs, nin, r, want, gt_want, part_want = case(n)
    c = ctxs[k]
    s0 = c.stats()
    sts, gt = c.verify_batch(proofs, kinds, inputs, nin, r=r, want_gt=True)
    s1 = c.stats()
    # the grid layout under test: K4 (cglv = 0) with ZG_K4_MIN = 1, the GLV C sums (cglv = 1) by default
    assert s1["glv_csum_batches"] - s0["glv_csum_batches"] == (0 if "ZG_K4_MIN" in ENVS[k] else 1)
    assert sts == want
    assert gt == gt_want
    part, sts = partial_of(c, proofs, kinds, inputs, nin, r, n)
    assert sts == want
    assert part == part_want


_BAD_POINTS = None
_BAD_PART = {}


def bad_points():
    """compressed curve points outside G1: (0, 2) of order 3, and the fixture's"""
    global _BAD_POINTS
    if _BAD_POINTS is None:
        o3 = B.g1_compress((0, 2))
        fx = bytes.fromhex(load_golden("points.json")["g1_not_in_subgroup"])
        for enc in (o3, fx):
            with pytest.raises(B.DecodeError):
                B.g1_decompress(enc)
        x = int.from_bytes(bytes([o3[0] & 0x1F]) + o3[1:], "big")
        assert x == 0 and o3[0] & 0x80
        _BAD_POINTS = {"order3": o3, "fixture": fx}
    return _BAD_POINTS


def bad_base():
    its = cut(BAD_N, only_ok=True)
    proofs, kinds, inputs, nin = fx_batch(its)
    r = b"".join(bytes.fromhex(e["r"]) for e in its)
    return its, proofs, kinds, inputs, nin, r


def bad_partial(slot):
    """the oracle's partial of the batch without the proof in `slot` (which proof of the slot is bad, and
    how, does not matter to the others), formed once per slot"""
    if slot not in _BAD_PART:
        its, proofs, _, _, _, _ = bad_base()
        live = live_of(its, proofs)
        _BAD_PART[slot] = B.f12_to_bytes(G.batch_partial(_pvks(), live[:slot] + live[slot + 1:]))
    return _BAD_PART[slot]


@pytest.mark.parametrize("k", range(len(ENVS)), ids=IDS)
@pytest.mark.parametrize("slot", [0, 63, 64])
@pytest.mark.parametrize("coord", ["A", "C"])
@pytest.mark.parametrize("which", ["order3", "fixture"])
def test_point_outside_g1_in_one_lane(ctxs, k, slot, coord, which):
    its, proofs, kinds, inputs, nin, r = bad_base()
    pr = bytearray(proofs)
    off = 192 * slot + (0 if coord == "A" else 144)
    pr[off:off + 48] = bad_points()[which]
    pr = bytes(pr)
    e = its[slot]
    st, _ = G.verify_status(_pvks()[e["kind"]], pr[192 * slot:192 * slot + 192],
                            [int.from_bytes(bytes.fromhex(x), "little") for x in e["inputs"]])
    assert st == G.DECODE_INVALID
    want = [st if i == slot else 0 for i in range(BAD_N)]
    c = ctxs[k]
    assert c.verify_batch(pr, kinds, inputs, nin, r=r)[0] == want
    part, sts = partial_of(c, pr, kinds, inputs, nin, r, BAD_N)
    assert sts == want
    assert part == bad_partial(slot)
