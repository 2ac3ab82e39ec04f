"""CPU tier of the PGHR13 batch-check edge tests: the case builders of tests/pghr13_edges.py stand on
the oracle alone (every slot's status from the C++ restatement of the reference's check, equal to the
fixture's own), the lane maps restated from the kernels' comments cover every proof exactly once, and
the positions and mutant classes the GPU tier runs reach what they are meant to reach."""
import itertools

import pytest

from tests import pghr13_edges as E


def _bk(env, n):
    s = E.expected_shape(env, n)
    return s["straus_b"], s["bseg_k"]


def _all_cases():
    out = E.nothing_live()
    for n in E.SWEEP_SIZES:
        out += [E.all_valid(n)] + E.excluded(n)
        for env in E.SHAPES + [E.UNSEEDED_SHAPE]:
            out += E.position_sweep(n, *_bk(env, n))
    for n in E.LARGE_SIZES:
        out += [E.all_valid(n), E.large_bad(n)]
    for n in E.CHUNK_SIZES:
        out += [E.all_valid(n)] + [E.one_bad(n, p, E.mutant_class(n, q)) for q, p in enumerate(E.chunk_positions(n))]
    return out + [E.large_bad(E.DEFAULT_CHUNK + 3)]


def test_slot_statuses_come_from_the_oracle_and_equal_the_fixture():
    """every slot the builders place: tests/cpulib.pg_verify's status is the fixture's own; the five
    mutants and nothing else fail the check, the excluded ones never reach it"""
    st, sl = E.oracle_statuses(), E.slots()
    assert set(st) == set(sl) and len(sl) == 9 + len(E.MUTANTS) + 2
    for k, (_, _, fixture) in sl.items():
        assert fixture is None or st[k] == fixture, k
    assert all(st["valid%d" % i] == E.OK for i in range(9))
    assert [st[m] for m in E.MUTANTS] == [E.VERIFY_FAILED] * 5
    assert st[E.DECODE_BAD] == E.DECODE_INVALID and st[E.NONCANON] == E.INPUT_NONCANONICAL
    assert sl[E.NONCANON][2] is None and sl[E.NONCANON][0] == sl["valid0"][0]


def test_built_cases_have_the_statuses_of_their_slots():
    sl = E.slots()
    for c in _all_cases():
        assert c.n == len(c.names) and c.n > 0
        want = [sl[k][2] if sl[k][2] is not None else E.INPUT_NONCANONICAL for k in c.names]
        assert c.statuses == want, c.name
        assert c.fails == (E.VERIFY_FAILED in want)
    c = E.one_bad(65, 64, 3)
    assert c.statuses == [0] * 64 + [3] and len(c.proofs) == 296 * 65 and len(c.inputs) == 288 * 65
    assert c.counts == bytes([9]) * 65
    assert E.all_valid(11).names[9] == "valid0"       # slot i holds valid case i mod 9
    for c in E.nothing_live():
        assert not set(c.statuses) & {E.OK, E.VERIFY_FAILED}
    assert [c.n for c in E.nothing_live()] == [1, 3, 65]
    for n in E.SWEEP_SIZES:
        for c in E.excluded(n):
            assert {c.names[0], c.names[-1]} <= {E.DECODE_BAD, E.NONCANON} and not c.fails


@pytest.mark.parametrize("per", [1, 2, 3, 4, 8, 32])
def test_lane_maps_partition_the_call(per):
    """g + k ceil(n / per) over lanes and strides is every proof exactly once, and no lane is empty"""
    for n in E.SWEEP_SIZES + E.LARGE_SIZES + E.CHUNK_SIZES + [3, 63, 64]:
        for lanes in (E.straus_slots(n, per), E.bseg_slots(n, per)):
            assert sorted(itertools.chain.from_iterable(lanes)) == list(range(n))
            assert len(lanes) == -(-n // per) and all(lanes) and all(len(l) <= per for l in lanes)
            assert [l[0] for l in lanes] == list(range(len(lanes)))


def test_shapes_and_sizes_are_the_issues():
    got = {(E.expected_shape(e, 521)["straus_b"], E.expected_shape(e, 521)["bseg_k"]) for e in E.SHAPES}
    assert got == {(1, 1), (2, 2), (1, 8), (4, 4), (2, 8), (4, 1), (4, 3), (1, 32)}
    assert E.SHAPES[0] == {} and _bk(E.UNSEEDED_SHAPE, 130) == (4, 8)
    assert E.SWEEP_SIZES == [1, 2, 5, 65, 130, 521] and E.LARGE_SIZES == [2063, 4099]
    assert sorted(E.VALID_ORDER) == sorted(E.SWEEP_SIZES + E.LARGE_SIZES)
    assert len(E.straus_slots(521, 4)) == 131 and len(E.bseg_slots(521, 8)) == 66      # 3 and 2 blocks of 64
    assert -(-2063 // 2) > 1024 and -(-4099 // 4) > 1024                                  # ZG_PGHR_SSUM_CH
    for env in E.CHUNK_ENVS:
        assert E.expected_shape(env, 200)["chunk"] == 64
    assert E.expected_shape({}, 1 << 20) == {"straus_b": 2, "bseg_k": 8, "halves": 1, "p7_side": 1, "chunk": 65536}
    assert E.expected_shape({}, 28672)["straus_b"] == 2 and E.expected_shape({}, 28671)["straus_b"] == 1
    assert [E.auto_shape(n)["bseg_k"] for n in E.THRESHOLD_SIZES] == [1, 1, 1, 2, 2, 2, 2, 4, 4, 8]


@pytest.mark.parametrize("env", E.SHAPES + [E.UNSEEDED_SHAPE], ids=E.shape_id)
def test_critical_positions_and_class_rotation(env):
    """per shape: the positions of every sweep size are distinct, within the call and hold n-1, 0 and the
    first slot of each map's last stride even when cut to 5; over the sweep and the large sizes slot n-1
    takes each of the five mutant classes"""
    last = set()
    for n in E.SWEEP_SIZES:
        b, k = _bk(env, n)
        pos = E.critical_positions(n, b, k)
        assert pos and len(pos) == len(set(pos)) <= E.MAX_POSITIONS and all(0 <= p < n for p in pos)
        keep = {p for p in (n - 1, 0, (b - 1) * -(-n // b), (k - 1) * -(-n // k)) if p < n}
        assert keep <= set(pos) and keep <= set(E.critical_positions(n, b, k, cap=5))
        # the last stride's first slot is the first slot of the last lane-stride of the restated map
        assert max(l[-1] for l in E.straus_slots(n, b)) == n - 1
        for c, p in zip(E.position_sweep(n, b, k), pos):
            assert c.statuses == [3 if i == p else 0 for i in range(n)]
            if p == n - 1:
                last.add(c.names[p])
    for n in E.LARGE_SIZES:
        c = E.large_bad(n)
        assert c.statuses == [0] * (n - 1) + [3]
        last.add(c.names[n - 1])
    assert last == set(E.MUTANTS)
    assert set(E.critical_positions(521, 4, 4)) == {520, 0, 393, 130, 131, 63, 64}
    assert E.chunk_positions(200) == [63, 64, 199, 192] and E.chunk_positions(64) == [63, 0]
    assert E.chunk_positions(65) == [63, 64] and E.chunk_positions(65539, 65536) == [63, 64, 65538, 65536]
