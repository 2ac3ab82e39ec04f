"""CPU tier: the case builders of tests/batch_edges.py build what they claim, by the oracle alone
(the C++ restatement of bellman's verify_proof for statuses, oracle/bls12_381.py for the group sums).
The GPU tier (tests/test_gpu_batch_edges.py) runs the same cases through every launch schedule."""
import collections

import pytest

from oracle import bls12_381 as B, groth16 as G
from tests import batch_edges as E


def test_schedules_cover_the_issue_list():
    """15 context knobs + 4 affine variants + fused 0 / 1 + default + GLV forced; no group of 2,048"""
    assert len(E.SCHEDULES) == 23
    assert {} in E.SCHEDULES and {"ZG_K4_MIN": 1 << 30} in E.SCHEDULES and {"ZG_K4_MIN": 1} in E.SCHEDULES
    assert {"ZG_LINES_FCHAIN": 0} in E.SCHEDULES and {"ZG_LINES_FCHAIN": 1} in E.SCHEDULES
    assert sorted(e["ZG_LINE_GROUP"] for e in E.SCHEDULES if "ZG_LINE_GROUP" in e) == \
        [0, 4, 4] + [32] * 8 + [128]
    affine = [e for e in E.SCHEDULES if any(k.startswith("ZG_LINES_AFFINE") for k in e)]
    assert len(affine) == 4 and all(e["ZG_LINE_GROUP"] == 32 and e["ZG_FCHAIN_QUADS"] == 1 for e in affine)
    assert all(e in E.SCHEDULES for e in E.MUTANT_SCHEDULES)


def test_expected_paths_at_the_clamps():
    """the library's own clamps restated: quads need npad >= 4, the group must fit, affine needs line
    products, fused excludes quads; every size of the sweep has padding except 1 -> 2 (none: 2)"""
    q32 = {"ZG_LINES_FCHAIN": 0, "ZG_FCHAIN_QUADS": 1, "ZG_LINE_GROUP": 32}
    aff = dict(q32, ZG_LINES_AFFINE=4)
    assert [E.npad_of(n) for n in E.SIZES] == [2, 2, 4, 8, 32, 64, 128, 256, 512]
    assert E.path_name(E.expected_path(q32, 2)) == "pairs/glv"
    assert E.path_name(E.expected_path(q32, 4)) == "quads/glv"
    assert E.path_name(E.expected_path(q32, 32)) == "lineprod/glv"
    assert E.path_name(E.expected_path(aff, 8)) == "quads/glv"
    assert E.path_name(E.expected_path(aff, 64)) == "affine+lineprod/glv"
    assert E.path_name(E.expected_path(dict(q32, ZG_LINE_GROUP=128), 64)) == "quads/glv"
    assert E.path_name(E.expected_path(dict(q32, ZG_LINE_GROUP=128), 128)) == "lineprod/glv"
    assert E.path_name(E.expected_path(dict(q32, ZG_LINE_GROUP=0), 512)) == "quads/glv"
    assert E.path_name(E.expected_path({}, 512)) == "fused/glv"
    assert E.path_name(E.expected_path({"ZG_K4_MIN": 1}, 2)) == "fused/k4"
    assert E.path_name(E.expected_path({"ZG_LINES_FCHAIN": 0}, 512)) == "pairs/glv"
    assert E.path_name(E.expected_path({"ZG_LINES_FCHAIN": 1, "ZG_FCHAIN_QUADS": 1}, 512)) == "fused/glv"


def test_pool_is_valid_and_cycles_over_all_sources():
    slots, rs = E.pool()   # (asserts that the oracle accepts every slot)
    assert len(slots) == len(rs) == E.POOL
    assert [s[0] for s in slots[:9]] == [0, 0, 1, 1, 1, 2, 2, 2, 2]
    assert len({s[1] for s in slots}) == 9 * E.VARIANTS and len(set(rs)) == E.POOL
    srcs = {bytes.fromhex(e["proof"]) for e in E.sources()}
    assert not srcs & {s[1] for s in slots}   # re-randomised, not the sources themselves


@pytest.mark.parametrize("n", E.SIZES)
def test_ragged_cases(n):
    """clean: all three keys present from n = 9 on, oracle statuses all 0; corrupted copy: exactly slot 0, one
    interior slot and slot n - 1 are rejected, nothing else"""
    c = E.ragged_clean(n)
    assert c.n == n and c.statuses == [0] * n
    assert set(c.kinds) == set([0, 0, 1, 1, 1, 2, 2, 2, 2][:n])
    if n >= 3:
        b = E.ragged_corrupt(n)
        bad = {i for i, s in enumerate(b.statuses) if s}
        assert bad == {0, n // 2, n - 1}
        assert all(b.statuses[i] in (1, 3) for i in bad)
        assert b.r == c.r and b.kinds == c.kinds


def test_ragged_corruptions_rotate_through_both_reject_classes():
    sts = collections.Counter(s for n in E.SIZES if n >= 3 for s in E.ragged_corrupt(n).statuses if s)
    assert sts[1] >= 3 and sts[3] >= 3
    # some batch must fail only by decode errors (no bisection) and some by a failed check (bisection)
    assert any(3 not in E.ragged_corrupt(n).statuses for n in E.SIZES if n >= 3)
    assert any(3 in E.ragged_corrupt(n).statuses for n in E.SIZES if n >= 3)


def test_minimal_bad_batches():
    assert [c.statuses for c in E.minimal_bad()] == [[3], [0, 3], [3, 0]]


@pytest.mark.parametrize("kinds", E.MIXES, ids=lambda k: "".join(map(str, k)))
def test_kind_mixes(kinds):
    for n in E.MIX_SIZES:
        c = E.mix_clean(kinds, n)
        assert set(c.kinds) == set(kinds) and c.statuses == [0] * n
        for k in {0, 1, 2} - set(kinds):
            assert c.c_terms(k) == []   # an absent key: an empty sum
        b = E.mix_corrupt(kinds, n)
        assert {i for i, s in enumerate(b.statuses) if s} == {0, n // 2, n - 1}


def test_mutant_batch_classes_and_oracle_agreement():
    """80 items: 48 x status 1, 17 x 3, 9 x 0, 3 x 2, 3 x 4; the C++ restatement agrees with the fixture on
    every status and every LHS GT"""
    f, o = E.mutant_batch(True), E.mutant_batch(False)
    assert f.n == 80 and f.npad == 128
    assert collections.Counter(f.statuses) == {1: 48, 3: 17, 0: 9, 2: 3, 4: 3}
    assert o.statuses == f.statuses
    assert len(f.live) == 26
    for i in range(f.n):
        assert (f._lhs[i] is not None) == (i in f.live)
        if i in f.live:
            assert o._lhs[i] == f._lhs[i], i
    assert f.nin == bytes(len(e["inputs"]) for e in E.mutant_items())


def test_mutant_rotations_put_every_class_first_and_last():
    base = E.mutant_batch()
    first, last = [], []
    for k in E.MUTANT_ROTATIONS:
        c = base.rotated(k)
        assert sorted(c.statuses) == sorted(base.statuses)
        assert c.proofs[:192] == base.proofs[192 * k:192 * k + 192] and c.r[-16:] == base.r16(k - 1)
        first.append(c.statuses[0])
        last.append(c.statuses[-1])
    assert first == [1, 2, 3, 4, 0] and last == [0, 1, 2, 3, 4]


@pytest.mark.parametrize("kind", sorted(E.DEGENERATE_KEYS))
def test_degenerate_sums(kind):
    """D1 - D4 by the oracle's own group arithmetic: the stated statuses; equal points meet in D1; the
    key's C-sum (batch_partial's csum[k], recomputed) or a node of its tree is the point at infinity in
    D2 - D4"""
    cases = E.degenerate_sums(kind)
    for name, c in cases.items():
        assert c.statuses == E.D_STATUSES[name], name
        t = c.c_tree(kind)
        assert t[1] == c.csum(kind), name   # the tree's root is the slot-order sum
        for k in {0, 1, 2} - {kind}:
            assert c.csum(k) is None
    rc = dict(cases["D3a"].c_terms(kind))
    rcp, rcq = rc[0], rc[2]
    assert rcp is not None and rcq is not None and rcp != rcq
    # D1: the two r_i C_i are equal points, their sum the doubling; one level up it doubles again
    terms = [p for _, p in cases["D1"].c_terms(kind)]
    assert terms[0] == terms[1] == rcp
    assert cases["D1"].csum(kind) == B.ec_mul(B.FQ, rcp, 2)
    t = cases["D1x4"].c_tree(kind)
    assert t[2] == t[3] == B.ec_mul(B.FQ, rcp, 2) and t[1] == B.ec_mul(B.FQ, rcp, 4)
    # D2: opposite points, the key's sum is infinity
    for name in ("D2", "D2rev"):
        terms = [p for _, p in cases[name].c_terms(kind)]
        assert terms[0] == B.ec_neg(B.FQ, terms[1]) and cases[name].csum(kind) is None
    # D3: infinity meets a point (left), or P and P' cancel around Q; right: infinity meets infinity
    t = cases["D3a"].c_tree(kind)
    assert t[2] is None and t[3] == rcq and t[1] == rcq
    for name in ("D3b", "D3c"):
        assert cases[name].csum(kind) == rcq
    t = cases["D3b"].c_tree(kind)
    assert t[2] == B.ec_add(B.FQ, rcq, rcp) and t[3] == B.ec_neg(B.FQ, rcp)
    t = cases["D3right"].c_tree(kind)
    assert t[2] is None and t[3] is None and t[1] is None
    # D4: a doubling meets its own half negated; two infinities
    t = cases["D4a"].c_tree(kind)
    assert t[2] == B.ec_mul(B.FQ, rcp, 2) and t[3] == B.ec_neg(B.FQ, rcp) and t[1] == rcp
    t = cases["D4b"].c_tree(kind)
    assert t[2] is None and t[3] is None and cases["D4b"].csum(kind) is None


def test_nothing_live():
    """D5: statuses all 1 (cpulib and the fixture agree); gt_out and the partial are the empty products"""
    one = G.batch_partial(E.pvks(), [])
    assert one == B.F12_ONE
    for c in E.nothing_live():
        assert c.statuses == [1] * c.n and c.live == []
        assert c.gt() == B.f12_to_bytes(B.F12_ONE) and c.partial() == B.f12_to_bytes(one)
    assert [c.n for c in E.nothing_live()] == [1, 3]
    assert E.nothing_live()[0].proofs == bytes(192)
    assert E.empty_batch().n == 0 and E.empty_batch().npad == 2
    assert E.empty_batch().gt() == E.empty_batch().partial() == B.f12_to_bytes(B.F12_ONE)


def test_extreme_scalars():
    """D6: the rows decode to the stated (a, b); a = b = 0 is r = 1; every proof stays valid"""
    c = E.extreme_scalars()
    assert c.n == 9 and c.npad == 16 and c.statuses == [0] * 9
    ab = [(int.from_bytes(c.r16(i)[:8], "little"), int.from_bytes(c.r16(i)[8:], "little")) for i in range(5)]
    m = (1 << 64) - 1
    assert ab == [(0, 0), (m, m), (m, 0), (0, m), (1 << 63, 1 << 63)]
    assert G.batch_r(c.r16(0)) == 1
    assert len({G.batch_r(c.r16(i)) for i in range(9)}) == 9


def test_extreme_inputs():
    """D7: the stated statuses, special slots first, last and interior; gt_out and the partial hold
    exactly the slots of status 0 and 3"""
    c = E.extreme_inputs()
    assert c.statuses == E.D7_STATUSES
    assert c.statuses[0] != 0 and c.statuses[-1] != 0 and 0 in c.statuses[1:-1]
    assert collections.Counter(c.statuses) == {0: 6, 3: 2, 4: 2, 2: 4}
    assert c.live == [i for i, s in enumerate(E.D7_STATUSES) if s in (0, 3)]
    row = lambda i: [int.from_bytes(c.inputs[288 * i + 32 * j:288 * i + 32 * j + 32], "little")  # noqa: E731
                     for j in range(G.KIND_NINPUTS[c.kinds[i]])]
    assert set(row(0)) == {0} and set(row(2)) == {B.R - 1}
    assert B.R in row(4) and (1 << 256) - 1 in row(5)
    own = [G.KIND_NINPUTS[k] for k in c.kinds]
    assert [c.nin[i] - own[i] for i in range(c.n)] == [0, 0, 0, 0, 0, 0, 0, -1, -1, 0, 0, 1, 0, 1]
    # the oracle's partial skips the same slots: dropping them from the batch changes nothing
    keep = E.Case("D7live", b"".join(c.proofs[192 * i:192 * i + 192] for i in c.live), bytes(c.kinds[i] for i in c.live),
                  b"".join(c.inputs[288 * i:288 * i + 288] for i in c.live), b"".join(c.r16(i) for i in c.live),
                  bytes(c.nin[i] for i in c.live))
    assert keep.partial() == c.partial() and keep.gt() == c.gt()
