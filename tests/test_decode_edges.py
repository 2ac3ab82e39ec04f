"""CPU tier of the point-decoder edge tests: the builders of tests/decode_edges.py build what they claim,
and every decoder that runs without a GPU holds the two rules on them -- the Python oracles, the C++
restatements (tests/cpulib) and the product's own decoders compiled for the host (tests/hostlib:
g1_decompress / g2_decompress, the uncompressed key decoders through vk_prepare, bn_g1_decode /
bn_g2_decode, jj_read, fq_lex_greatest / f2_lex_greatest), plus the host preparation functions of the
library. The GPU tier (tests/test_gpu_decode_edges.py) runs the same cases through the kernels."""
import collections
import ctypes

import pytest

from oracle import bls12_381 as B, groth16 as G, pghr13 as PG, sapling_sig as S, zcash as Z
from tests import batch_edges as E, cpulib, decode_edges as D, hostlib, pghr13_edges as PE

DEC_OK, DEC_ERR = 0, 2     # zg_curve.h


@pytest.fixture(scope="module")
def L():
    return hostlib.lib()


def fq_b(x):
    return x.to_bytes(48, "big")


def _proof(sp):
    return sp.slot[1]


def _ints(slot):
    return [int.from_bytes(x, "little") for x in slot[2]]


# ------------------------------------------------------------------ 1. Groth16 alias encodings
def test_alias_twins_cover_every_coordinate_and_key():
    """at least two twins per coordinate, all three keys among the twins, each twin its original with exactly
    one coordinate raised by p and the flag bits untouched; per coordinate one sign-flipped twin, its
    original and the sign-flipped original"""
    vs = D.variants()
    al = D.alias_specials()
    twins = [s for s in al if s.role == "alias" and " sign " not in s.name]
    per = collections.Counter(D.twin_source(s)[0] for s in twins)
    assert set(per) == set(D.COORDS) and min(per.values()) >= D.MIN_TWINS, per
    assert {s.slot[0] for s in twins} == {0, 1, 2}
    assert len({_proof(s) for s in al if s.role == "alias"}) == len([s for s in al if s.role == "alias"])
    for s in twins:
        c, i = D.twin_source(s)
        orig = vs[i][0][1]
        x = D.coord_get(orig, c)
        assert x < D.FQ_ROOM and D.coord_get(_proof(s), c) == x + B.P < 1 << 381
        assert D.coord_set(_proof(s), c, x) == orig
        off, fl = D.COORDS[c]
        assert _proof(s)[fl] & 0xE0 == orig[fl] & 0xE0
        assert [k for k in range(192) if _proof(s)[k] != orig[k]] and all(
            off <= k < off + 48 for k in range(192) if _proof(s)[k] != orig[k])
    for c in D.COORDS:
        extra = [s for s in al if s.name.startswith(c + "+p sign") or s.name.startswith(c + " original")]
        assert [s.status for s in extra] == [1, 0, 3], c
        fl = D.COORDS[c][1]
        assert _proof(extra[0])[fl] ^ 0x20 == D.coord_set(_proof(extra[1]), c, D.coord_get(_proof(extra[1]), c) + B.P)[fl]
        assert D.flip_sign(_proof(extra[1]), c) == _proof(extra[2])
    # the whole pool has room in every coordinate without further seeds only if this holds
    assert len(vs) >= D.NVARIANTS and [v[0] for v in vs[:D.NVARIANTS]] == E.pool()[0][:D.NVARIANTS]


def test_python_oracle_rejects_every_alias_twin_and_torsion_case():
    """G.proof_read: DecodeError for every special of status 1, a decoded proof for the others; the alias
    twins fail in the coordinate comparison itself (a reduced read of the same bytes decodes)"""
    for s in D.specials():
        if s.status == 1:
            with pytest.raises(B.DecodeError) as e:
                G.proof_read(_proof(s))
            want = "not in field" if s.role == "alias" else "NotInSubgroup"
            assert want in str(e.value), (s.name, str(e.value))
        else:
            G.proof_read(_proof(s))
    for s in D.alias_specials():
        if s.role == "alias":
            c, i = D.twin_source(s)
            reduced = D.coord_set(_proof(s), c, D.coord_get(_proof(s), c) - B.P)
            assert G.proof_read(reduced) is not None


def test_python_oracle_statuses_of_the_controls():
    """a subgroup point that is not the proof's: status 3 by oracle.groth16.verify_status, with the left-hand
    side the C++ restatement gives (the value gt_out takes)"""
    ctl = [s for s in D.torsion_specials() if s.role == "control"]
    assert [s.name for s in ctl] == ["A=[k]G", "C=[k]G", "B=[k]G"]
    case = E._from_slots("controls", [s.slot for s in ctl], b"".join(s.r for s in ctl))
    assert case.statuses == [3, 3, 3]
    for i, s in enumerate(ctl):
        st, gt = G.verify_status(E.pvks()[s.slot[0]], _proof(s), _ints(s.slot))
        assert st == G.VERIFY_FAILED and B.f12_to_bytes(gt) == case._lhs[i], s.name


@pytest.mark.parametrize("n", D.BATCH_SIZES)
def test_batches_hold_every_special_with_the_restatement_s_statuses(n):
    """the batches of one size hold every special exactly once, an alias twin first and a torsion case
    last, padded with valid pool proofs; tests/cpulib.verify gives each slot the status its construction
    states; gt_out runs over exactly the slots of status 0 and 3"""
    seen = []
    for case, who in D.groth16_batches(n):
        assert case.n == n == len(who)
        assert who[0].role == "alias" and who[-1].role == "torsion"
        assert case.statuses == D.expected_statuses(who), case.name
        assert case.live == [i for i, s in enumerate(who) if s is None or s.status in (0, 3)]
        assert 1 in case.statuses and 3 in case.statuses and who.count(None) >= 8
        seen += [s for s in who if s is not None]
    assert sorted(s.name for s in seen) == sorted(s.name for s in D.specials())
    for case, who in D.single_lane_cases():
        assert case.n == 1 and case.statuses == [1] and who[0].role in ("alias", "torsion")


def test_host_decoders_reject_alias_twins(L):
    """g1_decompress / g2_decompress compiled for the host: DEC_ERR on the twin's point, DEC_OK and the
    oracle's point on the original's"""
    vs = D.variants()
    out = hostlib.buf(192)
    for s in D.alias_specials():
        if s.role != "alias":
            continue
        c, i = D.twin_source(s)
        pos = c[0]
        off, ln = D.POINT_OFF[pos]
        fn = L.zgt_g2_decompress if pos == "B" else L.zgt_g1_decompress
        assert fn(_proof(s)[off:off + ln], out) == DEC_ERR, s.name
        orig = vs[i][0][1]
        assert fn(orig[off:off + ln], out) == DEC_OK, s.name
        pt = G.proof_read(orig)["ABC".index(pos)]
        want = b"".join(fq_b(v) for v in ((pt[0][0], pt[0][1], pt[1][0], pt[1][1]) if pos == "B" else pt))
        assert out.raw[:len(want)] == want


# ------------------------------------------------------------------ 2. cofactor torsion
def test_g2_torsion_set():
    """h2's identity holds (asserted in the builder); one point per prime part and Q + T each, none in G2
    by [r] P, of the stated order; two of them re-derived here from their definition"""
    cases = dict((nm, (p, ok)) for nm, p, ok in D.g2_torsion_cases())
    assert len(cases) == 2 * len(D.H2_PARTS) + 2
    assert cases["q"][1] and cases["generator"][1]
    q = cases["q"][0]
    for ell, e in D.H2_PARTS:
        t, ok = cases[D._g2_name(ell)]
        assert not ok and B.on_curve(B.FQ2, B.B2, t)
        assert t is not None and B.ec_mul(B.FQ2, t, ell ** e) is None
        qt, ok = cases["q_plus_" + D._g2_name(ell)]
        assert not ok and qt == B.ec_add(B.FQ2, q, t)
        assert B.ec_mul(B.FQ2, qt, B.R) == B.ec_mul(B.FQ2, t, B.R % ell ** e)
    # two points re-derived from the definition, with another random twist point: the same order
    import random
    rng = random.Random(0x63)
    for ell, e in D.H2_PARTS[:2]:
        while True:
            x = (rng.randrange(B.P), rng.randrange(B.P))
            y = B.f2_sqrt(B.f2_add(B.f2_mul(B.f2_sqr(x), x), B.B2))
            t = y and B.ec_mul(B.FQ2, (x, y), D.h2() * B.R // ell ** e)
            if t:
                break
        assert B.ec_mul(B.FQ2, t, ell ** e) is None and not B.g2_in_subgroup(t)


def test_torsion_placement():
    """every point outside its subgroup once per position it can take, the hosts over all three keys, only
    the placed point's bytes changed; the controls sit in the host of their position's first case"""
    to = D.torsion_specials()
    g1 = [nm for nm, _, ok in D.g1_torsion_cases() if not ok]
    g2 = [nm for nm, _, ok in D.g2_torsion_cases() if not ok]
    assert len(g1) == 12 and len(g2) == 12
    assert {"order_%d" % l for l in (3, 11, 10177, 859267, 52437899)} <= set(g1) and "order_3_0_2" in g1
    names = [s.name for s in to if s.role == "torsion"]
    assert names == ["A=" + n for n in g1] + ["C=" + n for n in g1] + ["B=" + n for n in g2]
    assert {s.slot[0] for s in to} == {0, 1, 2}
    hosts = {p for (_, p, _, _), _ in D.variants()}
    for s in to:
        pos = s.name[0]
        off, ln = D.POINT_OFF[pos]
        assert any(_proof(s)[:off] == h[:off] and _proof(s)[off + ln:] == h[off + ln:] and _proof(s) != h for h in hosts)
    for pos in "ACB":
        first = next(s for s in to if s.name.startswith(pos + "="))
        ctl = next(s for s in to if s.name == pos + "=[k]G")
        off, ln = D.POINT_OFF[pos]
        assert _proof(ctl)[:off] == _proof(first)[:off] and _proof(ctl)[off + ln:] == _proof(first)[off + ln:]
        assert ctl.r == first.r and ctl.status == 3 and first.status == 1


def test_host_decoders_reject_every_torsion_point(L):
    """g1_decompress / g2_decompress on the host: DEC_ERR for each compressed point outside its subgroup,
    DEC_OK for the subgroup points of the same sets"""
    out = hostlib.buf(192)
    for nm, p, ok in D.g1_torsion_cases():
        assert L.zgt_g1_decompress(B.g1_compress(p), out) == (DEC_OK if ok else DEC_ERR), nm
    for nm, p, ok in D.g2_torsion_cases():
        assert L.zgt_g2_decompress(B.g2_compress(p), out) == (DEC_OK if ok else DEC_ERR), nm


# ------------------------------------------------------------------ 3. PGHR13 alias encodings
def test_pghr13_twins_cover_every_point_and_multiple():
    """every G1 point with every k = 1 .. 4 (they always fit) and k = 5 wherever some valid case has room;
    b with every j = 1 .. 4 below 2^256; the q_big twin's quotient is at least 2^256 and its value below
    2^512; the wrap twins' quotients truncate to the valid c1"""
    tw = D.pghr13_twins()
    valid = D.pg_valid()
    what = [v[2] for v in tw.values()]
    assert D.PG_KMAX == 5 and 5 * D.BQ < 1 << 256 < 6 * D.BQ
    for point in D.PG_G1:
        fits5 = any(D.pg_g1_x(p, point) + 5 * D.BQ < 1 << 256 for _, p, _ in valid)
        want = [1, 2, 3, 4] + ([5] if fits5 else [])
        assert sorted(w[2] for w in what if w[:2] == ("g1", point)) == want, point
    fits5 = any(D.pg_b_u(p) // D.BQ + 5 * D.BQ < 1 << 256 for _, p, _ in valid)
    assert sorted(w[1] for w in what if w[0] == "c1") == [1, 2, 3, 4] + ([5] if fits5 else [])
    big = [w for w in what if w[0] == "big"]
    assert len(big) == 1 and big[0][2] >= 1 << 256
    assert sorted(w[1] for w in what if w[0] == "wrap") == [1, 4]
    by = {nm: p for nm, p, _ in valid}
    for name, (proof, ins, w) in tw.items():
        orig = by[name.split(":")[0]]
        diff = [k for k in range(296) if proof[k] != orig[k]]
        if w[0] == "g1":
            o = D.PG_G1[w[1]]
            assert diff and all(o + 1 <= k < o + 33 for k in diff)   # the sign byte stays
            assert D.pg_g1_x(proof, w[1]) == D.pg_g1_x(orig, w[1]) + w[2] * D.BQ
        else:
            assert diff and all(D.PG_B + 1 <= k < D.PG_B + 65 for k in diff)
            u, v = D.pg_b_u(orig), D.pg_b_u(proof)
            assert v % D.BQ == u % D.BQ and (v // D.BQ - u // D.BQ) % D.BQ in (0, (w[1] << 256) % D.BQ) and v < 1 << 512
            if w[0] == "c1":
                assert D.BQ <= v // D.BQ < 1 << 256
            else:
                assert v // D.BQ == w[2] >= 1 << 256


def test_pghr13_oracles_reject_every_twin(L):
    """oracle/pghr13.py: Proof::from_raw fails (INVALID_ENCODING) on every twin and not on the valid cases;
    the C++ restatement and the product's bn_g1_decode / bn_g2_decode on the host agree"""
    st = D.pghr13_statuses()
    out = hostlib.buf(128)
    for nm, proof, ins in D.pg_valid():
        assert st[nm] == PE.OK
        PG.proof_from_raw(proof)
        assert all(L.zgt_bn_g1_decode(proof[o:o + 33], out) == 1 for o in D.PG_G1.values())
        assert L.zgt_bn_g2_decode(proof[D.PG_B:D.PG_B + 65], out) == 1
    for name, (proof, ins, w) in D.pghr13_twins().items():
        with pytest.raises(PG.B.DecodeError):
            PG.proof_from_raw(proof)
        assert st[name] == PG.INVALID_ENCODING == PE.DECODE_INVALID, name
        if w[0] == "g1":
            o = D.PG_G1[w[1]]
            assert L.zgt_bn_g1_decode(proof[o:o + 33], out) == 0, name
        else:
            assert L.zgt_bn_g2_decode(proof[D.PG_B:D.PG_B + 65], out) == 0, name


def test_pghr13_cases():
    cases = D.pghr13_cases()
    assert [c.n for c in cases[:4]] == [1] * 4 and all(c.statuses == [1] for c in cases[:4])
    big = cases[-1]
    assert big.n > 64 and big.n % 64 and big.statuses[0] == big.statuses[-1] == 1 and not big.fails
    assert collections.Counter(big.statuses) == {1: len(D.pghr13_twins()), 0: big.n - len(D.pghr13_twins())}
    assert len(big.proofs) == 296 * big.n and len(big.inputs) == 288 * big.n and big.counts == bytes([9]) * big.n


# ------------------------------------------------------------------ 4. Jubjub alias encodings
def test_jubjub_small_y_points(L):
    """at least four multiples per generator with y < 2^255 - r; their alias y + r fits 255 bits, keeps
    the sign bit, and is rejected by Z.jubjub_read and by the kernels' jj_read on the host, which both
    read the canonical form to the oracle's point"""
    out = hostlib.buf(64)
    for gen, hits in D.jj_small_y().items():
        assert len(hits) >= D.JJ_MIN_POINTS, gen
        for k, enc in hits:
            x, y = Z.jubjub_read(enc)
            assert y < D.JJ_ROOM and not Z.is_small_order((x, y))
            al = D.jj_alias(enc)
            v = int.from_bytes(al, "little")
            assert v >> 255 == enc[31] >> 7 and v & ((1 << 255) - 1) == y + D.JR
            with pytest.raises(Z.PointError):
                Z.jubjub_read(al)
            assert L.zgt_jj_read(al, out) == 0, (gen, k)
            assert L.zgt_jj_read(enc, out) == 1
            assert out.raw == x.to_bytes(32, "little") + y.to_bytes(32, "little")


def test_redjubjub_alias_items():
    """the oracle accepts the four honest items and rejects the four alias items; an alias item differs
    from an accepted one only in the aliased encoding (key) or is the honest signature over the alias
    Rbar; a verifier that reduced the aliased bytes would accept each of them"""
    items = D.redjubjub_items()
    assert [i.ok for i in items] == [True, False, True, False] * 2
    for it in items:
        assert S.redjubjub_verify(it.vk, it.sig, it.msg, it.gen) == it.ok, it.name
    for good, bad in zip(items[0::4], items[1::4]):
        assert bad.vk == D.jj_alias(good.vk) and bad.sig == good.sig and bad.msg == good.msg
        assert bad.msg[:32] == good.vk                      # the message keeps the canonical key bytes
    for good, bad in zip(items[2::4], items[3::4]):
        assert bad.sig[:32] == D.jj_alias(good.sig[:32]) and bad.vk == good.vk and bad.msg == good.msg
        # reduced, the alias R is the honest R and the equation holds with the c of the alias bytes
        r, vk = S.read(good.sig[:32]), S.read(bad.vk)
        c, s = S.h_star(bad.sig[:32], bad.msg), int.from_bytes(bad.sig[32:], "little")
        assert S.is_zero(S.add(S.add(S.mul(vk, c), r), S.neg(S.mul(S.GENERATORS[bad.gen], s))))
    for n in (1, 65):
        b = D.redjubjub_batch(n)
        assert len(b) == n and not b[0].ok and not b[-1].ok
        assert {i.name for i in items} <= {i.name for i in b} or n == 1


def test_prep_alias_jobs_on_the_host():
    """zg_prep_spend / zg_prep_output (the library's host functions): the oracle's rows for the small-y
    descriptions, the oracle's error for each field encoded as y + r"""
    from zebra_amd import zg
    zg.lib()
    jobs = D.prep_jobs()
    assert [j.want for j in jobs] == [None, None, "ValueCommitment(Invalid)", "RandomizedKey(Invalid)",
                                      "ValueCommitment(Invalid)", "EphemeralKey(Invalid)"]
    for j in jobs:
        fn = zg.prep_spend if j.kind == "spend" else zg.prep_output
        if j.want is None:
            assert fn(*j.args) == D.prep_oracle_rows(j), j.name
        else:
            with pytest.raises(zg.PrepError) as e:
                fn(*j.args)
            assert e.value.name == j.want, j.name


def test_bvk_alias_rows():
    rows = D.bvk_rows()
    assert [r[3] for r in rows] == [0, 1, 1] and rows[0][4] != bytes(32) and rows[1][4] == rows[2][4] == bytes(32)


# ------------------------------------------------------------------ 5. uncompressed key points, sign compare
def test_uncompressed_key_points_with_a_coordinate_plus_p(L):
    """a G1 x, a G1 y, a G2 x half and a G2 y half of the builtin keys raised by p: the Python oracle's
    loader, the C++ restatement's and the product's vk_prepare on the host all refuse the key, and load
    it unchanged"""
    cases = D.vk_alias_cases()
    assert len(cases) == 4
    C = cpulib.load()
    ab = ctypes.create_string_buffer(576)
    try:
        for name, kind, fields, ic in cases:
            raw = b"".join(fields[k] for k in D.VK_FIELDS)
            good_f, good_ic = cpulib.vk_fields(kind)
            assert raw != good_f or ic != good_ic
            with pytest.raises(B.DecodeError) as e:
                G.load_vk_json(D.vk_json_text(fields, ic))
            assert "not in field" in str(e.value), name
            assert C.zgcpu_vk_load(kind, raw, len(ic), b"".join(ic), ab) != 0, name
            assert L.zgt_vk_prepare(raw, len(ic), b"".join(ic), ab) != 0, name
            assert L.zgt_vk_prepare(good_f, len(good_ic), b"".join(good_ic), ab) == 0, name
            assert ab.raw == B.f12_to_bytes(E.pvks()[kind].alpha_g1_beta_g2)
    finally:
        for k in cpulib.VK_FILES:   # the restatement's keys are shared state
            f, ic = cpulib.vk_fields(k)
            assert C.zgcpu_vk_load(k, f, len(ic), b"".join(ic), ab) == 0


def test_lexicographic_sign_compare(L):
    """fq_lex_greatest / f2_lex_greatest against plain integer comparison: y > p - y, around (p - 1) / 2 in
    every limb; Fq2 by c1 unless c1 = 0, then by c0"""
    half = (B.P - 1) // 2
    vals = D.lex_fq_values()
    assert vals[:5] == [half, half + 1, 1, B.P - 1, 0] and len(vals) >= 5 + 22
    for y in vals:
        assert L.zgt_fq_lex_greatest(fq_b(y)) == int(y > (-y) % B.P) == int(y > half), hex(y)
    pairs = D.lex_f2_values()
    assert any(c1 == 0 and c0 > half for c0, c1 in pairs) and any(c1 == 0 and 0 < c0 <= half for c0, c1 in pairs)
    for c0, c1 in pairs:
        want = B.f2_cmp_gt((c0, c1), B.f2_neg((c0, c1)))
        assert want == ((c1 > half) if c1 else (c0 > half))
        assert L.zgt_f2_lex_greatest(fq_b(c0) + fq_b(c1)) == int(want), (hex(c0), hex(c1))
