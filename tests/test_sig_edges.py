"""CPU tier of the signature-kernel edge tests: the vectors of tests/sig_edges.py (read its docstring)
are what they claim to be, by the references alone -- oracle/sapling_sig.py, tests/ed25519_ref.py,
tests/ecdsa_ref.py. tests/test_gpu_sig_edges.py sends the same vectors through the kernels.

The reference verifiers run over a stated subset of the table items (sig_edges.subset_digits: every digit
of window 0 and of the top window, d in {1, 128, largest valid} of every other window) and over every
twin; the rest is right by construction, and the construction's algebra is asserted for EVERY entry:
the window bases are [2^(8 w)] G by the reference's own scalar multiplication, and each entry d of
window w adds up with entry 256 - d to the base of window w + 1."""
import pytest

from oracle import sapling_sig as S
from oracle import zcash as Z
from tests import ecdsa_ref as EC
from tests import ed25519_ref as ED
from tests import sig_edges as E


# ----------------------------------------------------------------------------- A. counts and construction
def test_entry_counts():
    assert (E.RJ_ENTRIES, E.GV_ENTRIES, E.ED_ENTRIES, E.ED_UNREADABLE, E.EC_ENTRIES) == (7919, 1912, 7936, 224, 8160)
    assert (E.RJ_TOP_D << 248) < S.RJ <= ((E.RJ_TOP_D + 1) << 248)
    assert (E.GV_TOP_D << 56) <= E.INT64_MAX < ((E.GV_TOP_D + 1) << 56)
    assert not ((E.ED_TOP_D << 248) >> 248) & 0xE0 and ((E.ED_TOP_D + 1) << 248 >> 248) & 0xE0
    assert (255 << 248) < EC.N
    rj, rj_twins = E.redjubjub_table_items()
    assert [sum(1 for i in rj if i.gen == g) for g in (0, 1)] == [7919, 7919] and len({i.name for i in rj}) == 2 * 7919
    assert len({i.sig for i in rj}) == 2 * 7919
    assert sorted((i.gen, w) for i in rj_twins for w in [int(i.name.split()[4])]) == \
        [(g, w) for g in (0, 1) for w in range(32)]
    gv = E.gv_table_rows()
    assert len(gv) == 2 * 1912 and len({r.value for r in gv}) == 2 * 1912 and len({r.bvk for r in gv}) == 2 * 1912
    assert all(E.INT64_MIN < r.value <= E.INT64_MAX and not r.spends and not r.outputs for r in gv)
    ed, ed_twins, ed_unreadable = E.ed25519_table_items()
    assert (len(ed), len(ed_twins), len(ed_unreadable)) == (7936, 32, 224) and len({i.sig for i in ed}) == 7936
    ec, ec_twins = E.ecdsa_table_items()
    assert (len(ec), len(ec_twins)) == (8160, 64) and len({i.msg for i in ec}) == 8160
    assert {len(i.pubkey) for i in ec} == {33, 65} and sum(len(i.pubkey) == 33 for i in ec) == 4080
    # the GPU tier's calls: none of them a whole number of waves
    assert all(n % 64 for n in (len(rj) + len(rj_twins), len(gv), len(ed) + len(ed_twins), len(ed_unreadable),
                                len(ec) + len(ec_twins)))


def _check_comb(pts, g, mul, add, eq, windows):
    """every entry of comb_points: bases by the reference's scalar multiplication, entries by complement"""
    for w in range(windows):
        assert eq(pts[w, 1], mul(g, 1 << (8 * w))), w
        nxt = pts[w + 1, 1] if w + 1 < windows else mul(g, 1 << (8 * w + 8))
        for d in range(1, 256):
            assert eq(add(pts[w, d], pts[w, 256 - d]), nxt), (w, d)
        assert eq(pts[w, 255], mul(g, 255 << (8 * w))), w


def test_comb_algebra_jubjub():
    for gen, g in ((0, S.SPENDING_KEY_GENERATOR), (1, S.VALUE_COMMITMENT_RANDOMNESS), (2, S.VALUE_COMMITMENT_VALUE)):
        _check_comb(E.jj_comb(gen), g, S.mul, S.add, S.eq, 32 if gen < 2 else 8)


def test_comb_algebra_ed25519():
    def eq(p, q):
        return (p[0] * q[2] - q[0] * p[2]) % ED.P == 0 and (p[1] * q[2] - q[1] * p[2]) % ED.P == 0
    _check_comb(E.ed_comb(), ED.B, lambda p, k: ED.mul(k, p), ED.add, eq, 32)


def test_table_items_carry_their_point():
    """every entry: the key is the identity, S is the one digit of the name, and the R bytes are the
    reference's own encoding of comb point (w, d) (whose algebra the two tests above assert)"""
    rj, _ = E.redjubjub_table_items()
    for i in rj:
        _, _, g, _, w, _, d = i.name.split()
        assert i.vk == E.JJ_IDENTITY and int.from_bytes(i.sig[32:], "little") == int(d) << (8 * int(w)) < S.RJ
        assert i.sig[:32] == S.encode(E.jj_comb(int(g))[int(w), int(d)]), i.name
    assert S.is_zero(S.read(E.JJ_IDENTITY))
    ed, _, unreadable = E.ed25519_table_items()
    for i in ed + unreadable:
        _, _, w, _, d = i.name.split()
        assert i.pubkey == E.ED_IDENTITY and int.from_bytes(i.sig[32:], "little") == int(d) << (8 * int(w))
        assert bool(i.sig[63] & 0xE0) == (i.status == ED.SIGNATURE_ENCODING)
        assert i.sig[:32] == ED.compress(E.ed_comb()[int(w), int(d)]), i.name
    assert ED.decompress(E.ED_IDENTITY) == ED.IDENTITY


def test_ecdsa_items_have_one_digit_u1():
    """u1 = z / s is the digit and u1 + u2 k = t, for every entry; the twins keep u1 and miss t"""
    ec, twins = E.ecdsa_table_items()
    q = EC.mul(E.EC_KEY, EC.G)
    r = EC.mul(E.EC_NONCE, EC.G)[0] % EC.N
    for i in ec + twins:
        w, d = int(i.name.split()[2]), int(i.name.split()[4])
        assert EC.parse_pubkey(i.pubkey) == q
        rr, s = EC.parse_der_lax(i.sig)
        si = pow(s, -1, EC.N)
        u1, u2 = int.from_bytes(i.msg, "big") * si % EC.N, rr * si % EC.N
        assert rr == r and u1 == d << (8 * w), i.name
        assert ((u1 + u2 * E.EC_KEY) % EC.N == E.EC_NONCE) == (i.status == EC.OK), i.name
    assert any(EC.parse_der_lax(i.sig)[1] > EC.N // 2 for i in ec) and any(EC.parse_der_lax(i.sig)[1] <= EC.N // 2 for i in ec)


# ----------------------------------------------------------------------------- A. the reference verifiers, stated subset
def test_redjubjub_table_subset_and_twins_by_the_oracle():
    rj, twins = E.redjubjub_table_items()
    sub = E.rj_table_subset(rj)
    assert len(sub) == 2 * (255 + 14 + 30 * 3)
    for i in sub + twins:
        assert E.rj_oracle(i) == i.ok, i.name
    assert len(twins) == 64 and not any(i.ok for i in twins)


def test_gv_rows_subset_by_the_oracle():
    rows = E.gv_table_rows()
    sub = E.gv_table_subset(rows)
    assert len(sub) == 2 * (255 + 127 + 6 * 3)
    for r in sub:
        assert r.bvk == S.encode(S.neg(S.value_balance_point(r.value))), r.name
        assert E.bvk_expect([], [], r.value) == (0, r.bvk), r.name


def test_ed25519_table_subset_twins_and_unreadable_by_the_reference():
    ed, twins, unreadable = E.ed25519_table_items()
    sub = E.ed_table_subset(ed)
    assert len(sub) == 255 + 31 + 30 * 3
    for i in sub + twins + unreadable:
        assert ED.verify(i.pubkey, i.sig, i.msg) == i.status, i.name
    assert {i.status for i in twins} == {ED.SIGNATURE} and {i.status for i in unreadable} == {ED.SIGNATURE_ENCODING}
    assert sorted(int(i.name.split()[4]) for i in unreadable) == list(range(32, 256))


def test_ecdsa_table_subset_and_twins_by_the_reference():
    ec, twins = E.ecdsa_table_items()
    sub = E.ec_table_subset(ec)
    assert len(sub) == 2 * 255 + 30 * 3
    for i in sub + twins:
        assert EC.verify(i.pubkey, i.sig, i.msg) == i.status, i.name
    assert {i.status for i in twins} == {EC.SIGNATURE}


# ----------------------------------------------------------------------------- B. RedJubjub named items
def test_torsion_generator():
    y, t = E.torsion_generator()
    assert y == 11
    assert S.is_zero(S.mul(t, 8)) and not S.is_zero(S.mul(t, 4))
    assert len({S.encode(S.mul(t, k)) for k in range(8)}) == 8


def test_redjubjub_named_items_by_the_oracle():
    items = E.redjubjub_named_items()
    assert len({i.name for i in items}) == len(items) == 2 * (3 + 3 + 4 + 1)
    for i in items:
        assert E.rj_oracle(i) == i.ok, i.name
    # the torsion items stop testing the cofactor the day the equation without it accepts them
    torsion = [i for i in items if i.name.startswith("torsion")]
    assert len(torsion) == 12 and all(i.ok for i in torsion)
    for i in torsion:
        assert not E.redjubjub_verify_no_cofactor(i.vk, i.sig, i.msg, i.gen), i.name
    # ... and that equation is the oracle's but for the cofactor: it agrees on everything else here
    for i in items:
        if i not in torsion:
            assert E.redjubjub_verify_no_cofactor(i.vk, i.sig, i.msg, i.gen) == i.ok, i.name
    zero = [i for i in items if i.name.startswith("honest S = 0")]
    assert len(zero) == 2 and all(i.sig[32:] == bytes(32) and i.vk != E.JJ_IDENTITY for i in zero)


def test_redjubjub_gen_byte_items():
    items = E.redjubjub_gen_byte_items()
    assert len(items) == 2 * (2 + len(E.GEN_BYTES))
    for i in items:
        made_for = int(i.name.split()[3].rstrip(","))
        assert S.redjubjub_verify(i.vk, i.sig, i.msg, made_for)
        assert i.ok == ((1 if i.gen == 1 else 0) == made_for) == E.rj_oracle(i), i.name
    assert sum(i.ok for i in items) == 1 + len(E.GEN_BYTES) + 1


def test_redjubjub_size_batches():
    batches = E.redjubjub_size_batches()
    assert [len(b) for b in batches] == [0, 1, 1, 63, 64, 65, 129]
    for b in batches[1:]:
        assert b[0].name.startswith("torsion") or len(b) == 1
        assert not b[-1].ok or len(b) == 1
        for i in (b[0], b[-1]):
            assert E.rj_oracle(i) == i.ok, i.name
    assert batches[1][0].ok and not batches[2][0].ok


# ----------------------------------------------------------------------------- C. bvk rows and decode points
def test_bvk_batches():
    batches = E.bvk_batches()
    assert [len(b) for b in batches] == list(E.SIZES)
    assert len({b[-1].name for b in batches}) == len(batches)
    for rows in batches:
        n = len(rows)
        assert rows[-1].status != 0 and all(len(r.spends) + len(r.outputs) <= 5 for r in rows)
        for r in rows:
            assert (r.bvk == bytes(32)) == (r.status != 0), r.name
        if n < 63:
            continue
        assert {len(r.spends) + len(r.outputs) for r in rows} == set(range(6))
        assert not rows[0].spends and rows[0].outputs and rows[1].spends and not rows[1].outputs
        assert rows[3].bvk == E.JJ_IDENTITY
        assert rows[4].spends == rows[4].outputs and rows[4].spends and \
            rows[4].bvk == S.encode(S.neg(S.value_balance_point(rows[4].value)))
        assert (rows[5].value, rows[6].value) == (E.INT64_MIN + 1, E.INT64_MAX)
        assert Z.is_small_order(Z.jubjub_read(rows[7].spends[0])) and rows[7].status == 0
        assert [rows[i].status for i in range(10, 18)] == [1, 0, 1, 0, 2, 0, 1, 0]
        with pytest.raises(Z.PointError):
            Z.jubjub_read(rows[10].outputs[-1])
        with pytest.raises(Z.PointError):
            Z.jubjub_read(rows[12].spends[0])
        assert all(rows[i].status == 0 for i in (0, 1, 2, 3, 4, 5, 6, 7))
        if n > 64:
            assert [rows[i].status for i in (62, 63)] == [1, 2]
        if n > 65:
            assert rows[64].status == 0
    assert {r.status for rows in batches for r in rows} == {0, 1, 2}


def test_decode_batches():
    special = E.decode_special_points()
    # 24 encodings of 13 different strings: -[k]T is [8 - k]T, y = 0, 1, r - 1 are torsion points too
    assert len(special) == 24 and len(set(special)) == 13
    want = [E.decode_expect(p) for p in special]
    assert all(st == 2 for st, _, _ in want[:16])                      # both sign-bit forms of all 8 decode
    assert sorted({(x, y) for _, x, y in want[:16]}) == sorted(S.aff(S.mul(E.torsion_generator()[1], k)) for k in range(8))
    assert [st for st, _, _ in want[16:]] == [2, 2, 2, 1, 1, 1, 2, 2]   # y = 0, 1, r - 1 | r, r + 1, 2^255 - 1 | 1, r - 1 with bit 255
    batches = E.decode_batches()
    assert [len(p) for p, _ in batches] == list(E.SIZES)
    for pts, exp in batches:
        assert all((x, y) == (0, 0) for st, x, y in exp if st == 1)
        if len(pts) >= 63:
            assert pts[:24] == special
            assert {st for st, _, _ in exp} == {0, 1, 2}
    assert {exp[-1][0] for pts, exp in batches if len(pts) > 1} == {1, 2}
