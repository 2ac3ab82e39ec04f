"""The secp256k1 ECDSA check of transparent inputs on the GPU (zg_ecdsa_verify).

CPU tier: the big-int restatement (tests/ecdsa_ref.py) against the reference's key-pair vectors and
legacy-sighash transactions, every fixture status recomputed, the kernel's own per-item routine
compiled for the host (tests/native/zg_hosttest_ecdsa.hip) bit-exact on every fixture and on the
two field products, the collector's error precedence with injected verifiers, the corrupted-batch
expectation, and the kernel resource guard.
GPU tier: zg_ecdsa_verify against the fixture statuses (bit-exact verdict and error class), the
wave tail and second-block sizes, empty and longest signatures at the buffer's ends, a 4,097-item
batch with 1 % corrupted items, the field / scalar debug products, and the collector through a
real context."""
import ctypes
import os
import random
import shutil
import subprocess
import tempfile

import pytest

from tests import ecdsa_ref as E
from tests.conftest import load_golden

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST_SRC = os.path.join(HERE, "native", "zg_hosttest_ecdsa.hip")
HOST_LIB = os.path.join(HERE, "native", "libzg_hosttest_ecdsa.so")
CSRC = os.path.join(ROOT, "zebra_amd", "csrc")

needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")


def h(x):
    return bytes.fromhex(x)


_FIX = None


def fixture_items():
    """(name, pubkey, sig, msg, status) of real + signed + edges, computed once"""
    global _FIX
    if _FIX is None:
        g = load_golden("ecdsa.json")
        out = [(e["name"], h(e["pubkey"]), h(e["sig"]), h(e["sighash"]), e["status"]) for e in g["real"]]
        out += [("signed_%d" % i, h(e["pubkey"]), h(e["sig"]), h(e["msg"]), 0) for i, e in enumerate(g["signed"])]
        out += [(e["name"], h(e["pubkey"]), h(e["sig"]), h(e["msg"]), e["status"]) for e in g["edges"]]
        _FIX = out
    return _FIX


def run(ctx, items):
    return ctx.ecdsa_verify([i[1] for i in items], [i[2] for i in items], [i[3] for i in items])


def field_pairs(field):
    edge = [0, 1, E.P - 1, E.P, E.N - 1, E.N, 2 ** 255, 2 ** 256 - 1]
    rnd = random.Random(70 + field)
    return [(a, b) for a in edge for b in edge] + [(rnd.randrange(2 ** 256), rnd.randrange(2 ** 256))
                                                   for _ in range(256)]


def check_products(field, pairs, got):
    mod = E.P if field == 7 else E.N
    for (a, b), g in zip(pairs, got):
        assert int.from_bytes(g, "little") == a * b % mod, (field, hex(a), hex(b))


# ------------------------------------------------------------------ CPU tier
def test_helper_reference_vectors():
    g = load_golden("ecdsa.json")
    real = {e["name"]: e for e in g["real"]}
    assert len(real) == 14
    for e in real.values():
        assert E.verify(h(e["pubkey"]), h(e["sig"]), h(e["sighash"])) == e["status"], e["name"]
    # keys/src/keypair.rs:173-181: SIGN_1 / SIGN_2 under the uncompressed and the compressed key ...
    very, empty = E.dhash256(b"Very deterministic message"), E.dhash256(b"")
    for k in ("secret_1_sign_1", "secret_1c_sign_1", "secret_2_sign_2", "secret_2c_sign_2"):
        e = real["keypair_" + k]
        assert (h(e["sighash"]), e["status"], len(h(e["pubkey"]))) == (very, E.OK, 33 if "c_" in k else 65)
    # ... and not over dhash256("") (:180)
    for k in ("secret_2c", "secret_1"):
        e = real["keypair_%s_empty_message" % k]
        assert (h(e["sighash"]), e["status"]) == (empty, E.SIGNATURE)
    # script/src/interpreter.rs:1817-1907
    ok = ["p2pkh_3f285f08", "p2pk_high_s_12b5633b", "lax_der_fb0a1d8d", "compressed_key_54fabd73"]
    assert all(real[k]["status"] == E.OK for k in ok)
    assert E.parse_der_lax(h(real["p2pk_high_s_12b5633b"]["sig"]))[1] > E.N // 2          # normalize_s
    assert real["lax_der_fb0a1d8d"]["sig"].startswith("3048022200002b83")              # from_der_lax only
    assert len(h(real["compressed_key_54fabd73"]["pubkey"])) == 33
    multi = sorted(k for k in real if k.startswith("multisig_02b08211"))
    assert len(multi) == 4
    assert all(real[k]["status"] == (E.SIGNATURE if k.endswith("_mismatch") else E.OK) for k in multi), multi
    assert sum(1 for k in multi if k.endswith("_mismatch")) == 2
    assert len({real[k]["pubkey"] for k in multi}) >= 3


def test_fixture_statuses_recomputed():
    items = fixture_items()
    g = load_golden("ecdsa.json")
    assert (len(g["real"]), len(g["signed"])) == (14, 64)
    for name, pk, sg, m, st in items:
        assert E.verify(pk, sg, m) == st, name
    edges = [e["status"] for e in g["edges"]]
    assert all(edges.count(k) >= 8 for k in range(4)), [edges.count(k) for k in range(4)]
    signed = g["signed"]
    assert sum(1 for e in signed if len(h(e["pubkey"])) == 33) == 32
    assert sum(1 for e in signed if E.parse_der_lax(h(e["sig"]))[1] > E.N // 2) == 16
    want = {"key_len_0": 1, "key_len_66": 1, "key_x_plus_p_compressed": 1, "key_hybrid_right_parity": 0,
            "key_hybrid_wrong_parity": 1, "key_parity_swapped": 3, "sig_empty": 2, "sig_truncated_8": 2,
            "sig_seq_long_form_wrong_value": 0, "sig_8_length_bytes": 2, "sig_trailing_bytes": 0,
            "sig_top_bit_unpadded": 0, "sig_r_33_significant_bytes": 3, "sig_r_eq_n": 3, "sig_s_eq_n": 3,
            "arith_x_ge_n_second_compare": 0, "arith_r_plus_n_ge_p": 3, "arith_q_eq_g_doubling": 0,
            "arith_q_eq_neg_g_infinity": 3, "arith_u1g_eq_u2q": 0, "arith_m_plus_rd_zero_infinity": 3,
            "arith_zero_message": 0, "arith_message_ge_n": 0}
    got = {i[0]: i[4] for i in items}
    for name, st in want.items():
        assert got[name] == st, name


_HOST = None


def host_lib():
    """the kernel's per-item routine and field products compiled for the CPU (--offload-host-only),
    built on demand like tests/hostlib.py"""
    global _HOST
    if _HOST is None:
        deps = [HOST_SRC] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
        if not os.path.exists(HOST_LIB) or any(os.path.getmtime(d) > os.path.getmtime(HOST_LIB) for d in deps):
            subprocess.check_call(["hipcc", "-x", "hip", "--offload-host-only", "-O2", "-fPIC", "-shared",
                                   "-std=c++17", "-Wno-psabi", HOST_SRC, "-o", HOST_LIB])
        _HOST = ctypes.CDLL(HOST_LIB)
    return _HOST


def host_verify(items):
    from zebra_amd import zg
    keys, lens, sigs, off, msg = zg.pack_ecdsa([i[1] for i in items], [i[2] for i in items], [i[3] for i in items])
    st = ctypes.create_string_buffer(max(1, len(items)))
    assert host_lib().zgt_ecdsa_verify(ctypes.c_size_t(len(items)), keys, lens, sigs + b"\0", off, msg, st) == 0
    return list(st.raw[:len(items)])


@needs_hipcc
def test_host_compiled_kernel_routine_on_every_fixture():
    items = fixture_items()
    got = host_verify(items)
    bad = [(i[0], i[4], g) for i, g in zip(items, got) if g != i[4]]
    assert not bad, bad


@needs_hipcc
@pytest.mark.parametrize("field", [7, 8])
def test_host_compiled_field_products(field):
    pairs = field_pairs(field)
    out = ctypes.create_string_buffer(32 * len(pairs))
    host_lib().zgt_ecdsa_field_mul(field, ctypes.c_size_t(len(pairs)), b"".join(a.to_bytes(32, "little") for a, _ in pairs),
                                   b"".join(b.to_bytes(32, "little") for _, b in pairs), out)
    check_products(field, pairs, [out.raw[32 * i:32 * i + 32] for i in range(len(pairs))])


# ---- the collector: a window of transparent-only transactions and a P2PKH model of the script run
def real_checks():
    g = load_golden("ecdsa.json")
    real = {e["name"]: e for e in g["real"]}
    return [(h(real[k]["pubkey"]), h(real[k]["sig"]), h(real[k]["sighash"]))
            for k in ("p2pkh_3f285f08", "p2pk_high_s_12b5633b", "lax_der_fb0a1d8d")]


def p2pkh_rerun(checks, log=None):
    """the caller's second TransactionEval::check, modelled for inputs that are one OP_CHECKSIG each:
    the first input whose signature check is false is a Signature error with EvalFalse"""
    def rerun(lookup):
        if log is not None:
            log.append(len(checks))
        for c in checks:
            if not lookup(c.pubkey, c.sig, c.sighash):
                return ("Signature", c.input_index, "EvalFalse")
        return None
    return rerun


def ecdsa_window(log=None):
    from zebra_amd.collector import EcdsaCheck, Tx
    txs = []
    for k, (pk, sg, m) in enumerate(real_checks()):
        checks = [EcdsaCheck(input_index=k, pubkey=pk, sig=sg, sighash=m)]
        txs.append(Tx(ecdsa_checks=checks, eval_rerun=p2pkh_rerun(checks, log)))
    return txs


def flip(sig, at=9):
    return sig[:at] + bytes([sig[at] ^ 1]) + sig[at + 1:]


def ref_ecdsa(calls=None):
    def verify(pubkeys, sigs, msgs):
        if calls is not None:
            calls.append(len(pubkeys))
        return [E.verify(p, s, m) for p, s, m in zip(pubkeys, sigs, msgs)]
    return verify


def fake_verify(bad=()):
    def verify(proofs, kinds, inputs, n_inputs):
        return [2 if i in bad else 0 for i in range(len(kinds))]
    return verify


def test_collector_precedence_with_injected_verifiers():
    from tests.test_collector import fields, make_tx
    from zebra_amd import zg
    from zebra_amd.collector import EcdsaCheck, verify_block
    calls, reruns = [], []
    assert verify_block(ecdsa_window(reruns), verify=fake_verify(), verify_ecdsa=ref_ecdsa(calls)) is None
    assert calls == [3] and reruns == []                 # ONE call for the window; all OK: no rerun
    for k in range(3):
        del calls[:], reruns[:]
        t = ecdsa_window(reruns)
        t[k].ecdsa_checks[0].sig = flip(t[k].ecdsa_checks[0].sig)
        assert verify_block(t, verify=fake_verify(), verify_ecdsa=ref_ecdsa(calls)) == (k, ("Signature", k, "EvalFalse"))
        assert calls == [3] and reruns == [1]            # the rerun's triples were all in the table
    # every non-zero status makes the check false
    for st in (zg.ECDSA_PUBLIC, zg.ECDSA_SIGNATURE_ENCODING, zg.ECDSA_SIGNATURE):
        assert verify_block(ecdsa_window(), verify=fake_verify(),
                            verify_ecdsa=lambda p, s, m, st=st: [0, st, 0]) == (1, ("Signature", 1, "EvalFalse"))
    # the rerun's value is used verbatim: None (the script passes all the same) is no error
    t = ecdsa_window()
    t[1].ecdsa_checks[0].sig = flip(t[1].ecdsa_checks[0].sig)
    t[1].eval_rerun = lambda lookup: None
    t[2].ecdsa_checks[0].sig = flip(t[2].ecdsa_checks[0].sig)
    assert verify_block(t, verify=fake_verify(), verify_ecdsa=ref_ecdsa()) == (2, ("Signature", 2, "EvalFalse"))
    # the eval error comes ahead of JoinSplitSignature / InvalidJoinSplit on the same transaction
    F = fields()
    pk, sg, m = real_checks()[0]
    for js_sig_ok, bad, later in ((False, (), "JoinSplitSignature"), (True, {0}, ("InvalidJoinSplit", 0))):
        tx = make_tx(["J2"], F)
        tx.js_sig_ok = js_sig_ok
        tx.ecdsa_checks = [EcdsaCheck(0, pk, sg, m)]
        tx.eval_rerun = p2pkh_rerun(tx.ecdsa_checks)
        assert verify_block([tx], verify=fake_verify(bad), verify_ecdsa=ref_ecdsa()) == (0, later)
        tx.ecdsa_checks[0].sig = flip(sg)
        assert verify_block([tx], verify=fake_verify(bad), verify_ecdsa=ref_ecdsa()) == (0, ("Signature", 0, "EvalFalse"))
    # a pre_error still wins, and the lowest failing index
    t = ecdsa_window()
    t[1].ecdsa_checks[0].sig = flip(t[1].ecdsa_checks[0].sig)
    t[1].pre_error = "Maturity"
    assert verify_block(t, verify=fake_verify(), verify_ecdsa=ref_ecdsa()) == (1, "Maturity")
    t = ecdsa_window()
    t[2].ecdsa_checks[0].sig = flip(t[2].ecdsa_checks[0].sig)
    t[1].pre_error = "Maturity"
    assert verify_block(t, verify=fake_verify(), verify_ecdsa=ref_ecdsa()) == (1, "Maturity")
    t[0].ecdsa_checks[0].sig = flip(t[0].ecdsa_checks[0].sig)
    assert verify_block(t, verify=fake_verify(), verify_ecdsa=ref_ecdsa()) == (0, ("Signature", 0, "EvalFalse"))
    # a lookup miss (OP_CHECKMULTISIG trying another pair) is verified in ONE further call
    del calls[:]
    t = ecdsa_window()
    t[0].ecdsa_checks[0].sig = flip(t[0].ecdsa_checks[0].sig)
    other = real_checks()[1]

    def multisig_rerun(lookup):
        c = t[0].ecdsa_checks[0]
        assert lookup(c.pubkey, c.sig, c.sighash) is False
        assert lookup(*other) is True and lookup(*other) is True      # in the table; asked twice, verified once
        assert lookup(other[0], flip(other[1]), other[2]) is False    # never asked for: a further call
        return ("Signature", 0, "EvalFalse")
    t[0].eval_rerun = multisig_rerun
    assert verify_block(t, verify=fake_verify(), verify_ecdsa=ref_ecdsa(calls)) == (0, ("Signature", 0, "EvalFalse"))
    assert calls == [3, 1]
    # checks without a backend raise; so does a failed check without eval_rerun
    with pytest.raises(zg.ZgError):
        verify_block(ecdsa_window(), verify=fake_verify())
    t = ecdsa_window()
    t[1].ecdsa_checks[0].sig = flip(t[1].ecdsa_checks[0].sig)
    t[1].eval_rerun = None
    with pytest.raises(zg.ZgError):
        verify_block(t, verify=fake_verify(), verify_ecdsa=ref_ecdsa())
    # transactions without checks ask for no call
    del calls[:]
    assert verify_block([make_tx(["J2"], F)], verify=fake_verify(), verify_ecdsa=ref_ecdsa(calls)) is None
    assert calls == []


_BATCH = None


def corrupted_batch(n=4097, seed=7):
    """the signed fixtures cycled to n, 1 % corrupted in rotating ways -> (items, expected); the
    expectation is computed once per distinct triple and shared by the CPU and the GPU test"""
    global _BATCH
    if _BATCH is not None:
        return _BATCH
    valid = [i for i in fixture_items() if i[0].startswith("signed_")]
    rnd = random.Random(seed)
    items = [list(valid[i % len(valid)]) for i in range(n)]
    memo = {}

    def expect(pk, sg, m):
        if (pk, sg, m) not in memo:
            memo[(pk, sg, m)] = E.verify(pk, sg, m)
        return memo[(pk, sg, m)]

    def flip_bit(b, lo, hi):
        k = rnd.randrange(8 * lo, 8 * hi)
        return b[:k // 8] + bytes([b[k // 8] ^ (1 << (k % 8))]) + b[k // 8 + 1:]

    for c, i in enumerate(sorted(rnd.sample(range(n), n // 100))):
        _, pk, sg, m, _ = items[i]
        r_len = sg[3]
        s_at = 4 + r_len + 2
        how = c % 8
        if how == 0:
            m = flip_bit(m, 0, 32)
        elif how == 1:
            sg = flip_bit(sg, 4, 4 + r_len)
        elif how == 2:
            sg = flip_bit(sg, s_at, len(sg))
        elif how == 3:
            pk = bytes([pk[0] ^ 1]) + pk[1:]                      # the parity byte
        elif how == 4:
            pk = flip_bit(pk, 1, 33)
        elif how == 5:
            sg = sg[:2] + bytes([sg[2] ^ (1 << rnd.randrange(8))]) + sg[3:]   # the DER tag of R
        elif how == 6:
            sg = sg[:s_at - 1] + bytes([sg[s_at - 1] + 1 + rnd.randrange(8)]) + sg[s_at:]   # S runs past the end
        else:
            r, s = E.parse_der_lax(sg)
            sg = E.der(r, E.N - s)                                # still valid
        items[i] = ["corrupt_%d" % how, pk, sg, m, None]
    want = [expect(i[1], i[2], i[3]) for i in items]
    _BATCH = (items, want)
    return _BATCH


def test_corrupted_batch_expectation():
    """the 4,097-item batch of the GPU test: its non-zero count for the chosen seed, here on the CPU"""
    items, want = corrupted_batch()
    assert len(items) == 4097
    nz = sum(1 for s in want if s)
    assert 20 <= nz <= 70, nz
    by_how = {}
    for i, w in zip(items, want):
        if i[0].startswith("corrupt_"):
            by_how.setdefault(int(i[0][8:]), set()).add(w)
    assert by_how[7] == {0} and by_how[5] == {2} and by_how[6] == {2} and by_how[0] == {3}, by_how
    assert sorted(by_how) == list(range(8))


@needs_hipcc
def test_host_compiled_kernel_routine_on_the_corruptions():
    items, want = corrupted_batch()
    bad = [(i, w) for i, w in zip(items, want) if i[0].startswith("corrupt_")]
    assert host_verify([i for i, _ in bad]) == [w for _, w in bad]


@needs_hipcc
def test_ecdsa_kernels_have_no_scratch():
    """k_ecdsa and k_ec_comb off the private segment, as k_ed25519 is"""
    from tools import resource_table
    with tempfile.TemporaryDirectory() as tmp:
        rows = {r["name"]: r for r in resource_table.unit("zg_ecdsa.hip", tmp) if "occ" in r}
    assert len(rows) == 2 and any("k_ecdsa" in n for n in rows) and any("k_ec_comb" in n for n in rows), sorted(rows)
    for name, r in rows.items():
        assert r["scratch"] == 0 and r.get("vspill", 0) == 0 and r["vgpr"] <= 256 and r["occ"] >= 2, (name, r)


# ------------------------------------------------------------------ GPU tier
@pytest.fixture(scope="module")
def ctx():
    from zebra_amd import Context
    return Context(device=0, max_batch=64, load_builtin=False)


@pytest.mark.gpu
def test_gpu_fixture_statuses(ctx):
    items = fixture_items()
    got = run(ctx, items)
    bad = [(i[0], i[4], g) for i, g in zip(items, got) if g != i[4]]
    assert not bad, bad


@pytest.mark.gpu
def test_gpu_sizes_wave_tail_and_second_block(ctx):
    items = fixture_items()
    edges = [i for i in items if i[4] != 0]
    assert run(ctx, []) == []
    for k, n in enumerate((1, 63, 64, 65, 129)):
        batch = [items[j % len(items)] for j in range(n)]
        batch[-1] = edges[(11 * k + 3) % len(edges)]   # a different non-zero edge case at the last index of each size
        got = run(ctx, batch)
        assert got == [b[4] for b in batch], n
    assert len({edges[(11 * k + 3) % len(edges)][0] for k in range(5)}) == 5


@pytest.mark.gpu
def test_gpu_empty_and_longest_signature_at_the_buffer_ends(ctx):
    items = fixture_items()
    empty = [i for i in items if i[0] == "sig_empty"][0]
    longest = max(items, key=lambda i: len(i[2]))
    assert len(empty[2]) == 0 and len(longest[2]) > 72
    mid = items[:30]
    for first, last in ((empty, longest), (longest, empty), (empty, empty), (longest, longest)):
        batch = [first] + mid + [last]
        assert run(ctx, batch) == [b[4] for b in batch]
    assert run(ctx, [empty]) == [2] and run(ctx, [empty, empty]) == [2, 2]


@pytest.mark.gpu
def test_gpu_corrupted_batch(ctx):
    items, want = corrupted_batch()
    got = run(ctx, items)
    assert got == want, [(i, w, g) for i, (w, g) in enumerate(zip(want, got)) if w != g][:8]
    assert 20 <= sum(1 for s in got if s) <= 70


@pytest.mark.gpu
@pytest.mark.parametrize("field", [7, 8])
def test_gpu_debug_field_products(field):
    from zebra_amd import zg
    pairs = field_pairs(field)
    got = zg.debug_field_mul(field, [a.to_bytes(32, "little") for a, _ in pairs],
                             [b.to_bytes(32, "little") for _, b in pairs])
    check_products(field, pairs, got)


@pytest.mark.gpu
def test_gpu_collector_real_context():
    from zebra_amd import Context
    from zebra_amd.collector import verify_block
    c = Context(device=0, max_batch=64)
    assert verify_block(ecdsa_window(), ctx=c) is None
    for k in range(3):
        t = ecdsa_window()
        t[k].ecdsa_checks[0].sig = flip(t[k].ecdsa_checks[0].sig, 20)
        assert verify_block(t, ctx=c) == (k, ("Signature", k, "EvalFalse"))
