"""Block-header checks, CPU tier: the byte-level restatement
(tests/equihash_ref.py) against the generated fixture (tests/golden/equihash.json: the 13 real
headers, the reference's (96, 5) vector, named (200, 9) mutants, crafted (48, 5) solutions on which
the reference and the specification differ), zg_pow_valid against the proof-of-work vectors, the
new symbols, and the deferred writer's error precedence with headers through a fake backend.
The GPU tier is tests/test_gpu_equihash.py."""
import itertools

import pytest

from tests import equihash_ref as Q
from tests.conftest import load_golden


def h(x):
    return bytes.fromhex(x)


_G = None


def fixture():
    global _G
    if _G is None:
        _G = load_golden("equihash.json")
    return _G


# ------------------------------------------------------------------ the restatement against the fixture
def test_real_headers_verify_and_hash():
    g = fixture()
    assert [e["height"] for e in g["real"]] == [0, 1, 2, 3, 9, 169, 170, 181, 182, 522, 567, 1033, 419221]
    assert g["max_bits"] == Q.MAINNET_MAX_BITS == 0x1f07ffff
    for e in g["real"]:
        hd = h(e["header"])
        assert len(hd) == Q.HEADER_BYTES and hd[140:143] == b"\xfd\x40\x05"
        assert Q.block_hash(hd) == h(e["hash"])
        assert Q.header_flags(hd, g["max_bits"])[0] == 0 and Q.header_status(hd, g["max_bits"]) == Q.HDR_OK
    # the genesis and block 1 hashes as the explorers print them
    assert h(g["real"][0]["hash"])[::-1].hex().startswith("00040fe8")
    assert h(g["real"][1]["hash"])[::-1].hex().startswith("0007bc22")
    # block 1 builds on the genesis block
    assert h(g["real"][1]["header"])[4:36] == h(g["real"][0]["hash"])


def test_reference_96_5_vector_and_swaps():
    r = fixture()["ref96"]
    assert Q.verify(96, 5, h(r["input"]), h(r["solution"]))
    assert len(r["swaps"]) == 5
    for s in r["swaps"]:
        assert not Q.verify(96, 5, h(r["input"]), h(s["solution"])), s["level"]


def test_mutants_recomputed():
    g = fixture()
    got = {}
    for m in g["mutants"]:
        hd = h(m["header"])
        f, hh = Q.header_flags(hd, g["max_bits"])
        assert (Q.header_status(hd, g["max_bits"]), f, hh) == (m["status"], m["flags"], h(m["hash"])), m["name"]
        assert m["status"] != Q.HDR_OK
        got[m["name"]] = (m["status"], m["flags"])
    assert set(got) == {"swap_level_%d" % l for l in range(9)} | {
        "index_xor_1", "leaf1_equals_leaf0", "nonce_bit", "solution_bit", "solution_last_bit", "bad_solution_length"}
    assert got["nonce_bit"] == (Q.HDR_EQUIHASH, Q.F_EQUIHASH | Q.F_POW)
    assert got["bad_solution_length"][0] == Q.HDR_MALFORMED
    assert got["leaf1_equals_leaf0"][1] & Q.F_REPEATED


def test_leaf1_equals_leaf0_is_rejected_by_distinct_indices_only():
    """the collision and the order check pass on the first pair; distinct_indices rejects it"""
    m = next(m for m in fixture()["mutants"] if m["name"] == "leaf1_equals_leaf0")
    hd = h(m["header"])
    p = Q.Params(200, 9)
    rows = Q.initial_rows(p, hd[:140], hd[143:])
    assert Q.has_collision(rows[0], rows[1], p.BSTR_INDEX_BYTES)
    assert not Q.indices_before(rows[1], rows[0], p.ROW_HASH_LENGTH, 4)
    assert not Q.distinct_indices(rows[0], rows[1], p.ROW_HASH_LENGTH, 4)


def test_crafted_solutions_reference_against_specification():
    g = fixture()
    c = g["crafted48"]
    assert sum(e["repeated"] for e in c) >= 3 and sum(1 - e["repeated"] for e in c) >= 4
    for e in c + g["boundary48"]:
        assert Q.verify(48, 5, h(e["input"]), h(e["solution"]))                       # the reference accepts all
        assert Q.strict_distinct(48, 5, h(e["solution"])) == (not e["repeated"])      # the specification does not
    assert [len(h(e["input"])) for e in g["boundary48"]] == [128, 129]
    assert all(len(h(e["input"])) == 56 for e in c)


def test_distinct_indices_compares_only_the_first_left_index():
    """rows of two indices each: a repeat of the left row's SECOND index goes unnoticed"""
    def row(a, b):
        return a.to_bytes(4, "big") + b.to_bytes(4, "big")
    assert Q.distinct_indices(row(1, 7), row(5, 7), 0, 8)
    assert not Q.distinct_indices(row(7, 1), row(5, 7), 0, 8)


def test_expand_array_and_compress_indices_round_trip():
    for n, k in ((200, 9), (96, 5), (48, 5)):
        p = Q.Params(n, k)
        idx = [(i * 2654435761) % (1 << (p.BSTR_INDEX_BITS + 1)) for i in range(1 << k)]
        sol = Q.compress_indices(p, idx)
        assert len(sol) == p.SOLUTION_COMPRESSED_SIZE == {200: 1344, 96: 68, 48: 36}[n]
        assert Q.solution_indices(p, sol) == idx


# ------------------------------------------------------------------ proof of work
def test_compact_vectors_of_the_reference():
    """primitives/src/compact.rs:109-117 (test_compact_to_u256)"""
    T = Q.compact_to_u256
    assert T(0x01003456) == (True, 0) and T(0x01123456) == (True, 0x12) and T(0x02008000) == (True, 0x80)
    assert T(0x05009234) == (True, 0x92340000) and T(0x04123456) == (True, 0x12345600)
    assert not T(0x04923456)[0]
    # as written: the word of a size <= 3 compact is shifted before the sign test
    assert T(0x01803456) == (True, 0) and not T(0x02803456)[0]


def test_pow_vectors_recomputed():
    v = fixture()["pow"]
    names = {e["name"] for e in v}
    assert {"size1_eq", "size2_above", "sign_zero_word", "sign_nonzero_word", "overflow_size35", "overflow_size34_word",
            "overflow_size33_word", "hash_eq_target", "hash_target_minus_1", "hash_target_plus_1", "target_above_max",
            "sign_as_max_bits", "overflow_as_max_bits"} <= names
    for e in v:
        assert Q.is_valid_proof_of_work(e["max_bits"], e["bits"], h(e["hash"])) == bool(e["valid"]), e["name"]
    byname = {e["name"]: e["valid"] for e in v}
    assert byname["hash_eq_target"] == 1 and byname["hash_target_minus_1"] == 1 and byname["hash_target_plus_1"] == 0
    assert byname["target_above_max"] == 0 and byname["target_eq_max"] == 1
    assert byname["sign_size1_word_shifted_out"] == 1 and byname["sign_size2_word_kept"] == 0


def test_zg_pow_valid_against_the_vectors():
    from zebra_amd import zg
    g = fixture()
    for e in g["pow"]:
        assert zg.pow_valid(e["max_bits"], e["bits"], h(e["hash"])) == bool(e["valid"]), e["name"]
    for e in g["real"]:
        hd = h(e["header"])
        bits = int.from_bytes(hd[104:108], "little")
        assert zg.pow_valid(g["max_bits"], bits, h(e["hash"]))
    with pytest.raises(zg.ZgError):
        zg.pow_valid(0, 0, b"\0" * 31)


def test_new_symbols_exported():
    from zebra_amd import zg
    L = zg.lib()
    for s in ("zg_equihash_verify", "zg_headers_verify", "zg_pow_valid"):
        assert hasattr(L, s), s
    assert (zg.EQ_200_9, zg.EQ_96_5, zg.EQ_48_5) == (0, 1, 2) and zg.HEADER_BYTES == 1487
    assert (zg.HDR_OK, zg.HDR_MALFORMED, zg.HDR_EQUIHASH, zg.HDR_POW) == (0, 1, 2, 3)
    assert (zg.HDR_F_EQUIHASH, zg.HDR_F_POW, zg.HDR_F_REPEATED) == (1, 2, 4)
    for name in ("equihash_verify", "headers_verify"):
        assert callable(getattr(zg.Context, name))


# ------------------------------------------------------------------ the writer's precedence (fake backend)
CHECKS = ("header_precheck", "equihash", "pow", "precheck", "tx")


class FakeTx:
    def __init__(self, err):
        self.err, self.joinsplits, self.spends, self.outputs = err, [0], [], []


def fake_block(i, fails, with_header=True):
    """block i on parent i - 1 failing the given checks; its header bytes carry the header verdict"""
    from zebra_amd.blocks_writer import Block
    st = Q.HDR_EQUIHASH if "equihash" in fails else Q.HDR_POW if "pow" in fails else Q.HDR_OK
    return Block(hash=i, parent=i - 1, txs=[FakeTx(None), FakeTx("InvalidSapling" if "tx" in fails else None)],
                 precheck=(lambda w: "FuturisticTimestamp") if "precheck" in fails else None,
                 header=bytes([st, i]) if with_header else None,
                 header_precheck=(lambda w: "InvalidVersion") if "header_precheck" in fails else None)


def expected_error(fails):
    """the reference's order inside one block"""
    for c, e in zip(CHECKS, ("InvalidVersion", "InvalidEquihashSolution", "Pow", "FuturisticTimestamp",
                             (1, "InvalidSapling"))):
        if c in fails:
            return e
    return None


def run_writer(blocks, **kw):
    """-> (inserted hashes, error detail | None, header calls, window calls)"""
    from zebra_amd.blocks_writer import DeferredBlocksWriter, MemoryStorage, WriterError
    calls = {"h": [], "w": 0}

    def verify_headers(headers):
        calls["h"].append(len(headers))
        return [x[0] for x in headers]

    def verify_window(txs):
        calls["w"] += 1
        for i, t in enumerate(txs):
            if t.err:
                return i, t.err
        return None

    st = MemoryStorage(0)
    w = DeferredBlocksWriter(st, verify_window=verify_window, verify_headers=verify_headers, **kw)
    err = None
    try:
        for b in blocks:
            w.append_block(b)
        w.flush()
    except WriterError as e:
        assert e.kind == "Verification"
        err = e.detail
    return st.blocks[1:], err, calls["h"], calls["w"]


def all_subsets():
    return [frozenset(c) for r in range(len(CHECKS) + 1) for c in itertools.combinations(CHECKS, r)]


def test_writer_precedence_within_one_block():
    for fails in all_subsets():
        ins, err, hcalls, _ = run_writer([fake_block(1, ()), fake_block(2, fails), fake_block(3, ())])
        want = expected_error(fails)
        assert err == want, (sorted(fails), err)
        assert ins == ([1, 2, 3] if want is None else [1]), (sorted(fails), ins)
        assert len(hcalls) <= 1                                   # ONE headers call per verified window
        if "header_precheck" not in fails:
            assert hcalls == [3 if not fails & {"precheck"} else 2]


def test_writer_precedence_across_two_blocks():
    """the lowest block wins whatever the kinds: every ordered pair of single failures"""
    for a in CHECKS:
        for b in CHECKS:
            ins, err, hcalls, _ = run_writer([fake_block(1, ()), fake_block(2, {a}), fake_block(3, {b})])
            assert err == expected_error({a}) and ins == [1], (a, b, err, ins)
            assert len(hcalls) <= 1
    # a header error of a LATER block does not hide an earlier block's transaction error, and the
    # transactions of blocks behind a failing header are not verified at all
    ins, err, _, wcalls = run_writer([fake_block(1, {"tx"}), fake_block(2, {"equihash"})])
    assert (ins, err, wcalls) == ([], (1, "InvalidSapling"), 1)
    ins, err, _, wcalls = run_writer([fake_block(1, {"pow"}), fake_block(2, {"tx"})])
    assert (ins, err, wcalls) == ([], "Pow", 0)


def test_writer_failed_precheck_still_verifies_its_header():
    """a block whose precheck fails at append flushes the window with its own header in the same call"""
    ins, err, hcalls, _ = run_writer([fake_block(1, ()), fake_block(2, {"precheck", "pow"})])
    assert (ins, err, hcalls) == ([1], "Pow", [2])
    ins, err, hcalls, _ = run_writer([fake_block(1, ()), fake_block(2, {"precheck"})])
    assert (ins, err, hcalls) == ([1], "FuturisticTimestamp", [2])
    # the window's own error still comes first
    ins, err, hcalls, _ = run_writer([fake_block(1, {"tx"}), fake_block(2, {"precheck", "equihash"})])
    assert (ins, err, hcalls) == ([], (1, "InvalidSapling"), [2])


def test_writer_windows_by_header_count():
    ins, err, hcalls, _ = run_writer([fake_block(i, ()) for i in range(1, 8)], window_headers=3)
    assert (ins, err, hcalls) == (list(range(1, 8)), None, [3, 3, 1])


def test_writer_without_headers_is_the_old_behaviour():
    """header=None: no headers call, header_precheck ignored, the same storage and error as the sequential
    writer over the same blocks"""
    from zebra_amd.blocks_writer import MemoryStorage, SequentialBlocksWriter, WriterError
    for fails in all_subsets():
        blocks = [fake_block(1, (), False), fake_block(2, fails, False), fake_block(3, (), False)]
        ins, err, hcalls, _ = run_writer(blocks)
        assert hcalls == []

        def check(b):
            pre = b.precheck(None) if b.precheck else None
            if pre is not None:
                return pre
            return next(((i, t.err) for i, t in enumerate(b.txs) if t.err), None)
        st = MemoryStorage(0)
        seq = SequentialBlocksWriter(st, check)
        want = None
        try:
            for b in blocks:
                seq.append_block(b)
        except WriterError as e:
            want = e.detail
        assert (ins, err) == (st.blocks[1:], want), sorted(fails)


def test_writer_needs_a_backend_for_headers():
    from zebra_amd.blocks_writer import DeferredBlocksWriter, MemoryStorage
    w = DeferredBlocksWriter(MemoryStorage(0), verify_window=lambda txs: None)
    w.append_block(fake_block(1, ()))
    with pytest.raises(RuntimeError):
        w.flush()
    assert w.window and not w.storage.blocks[1:]      # nothing taken, nothing inserted
