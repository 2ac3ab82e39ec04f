"""The Ed25519 JoinSplit signature check on the GPU (zg_ed25519_verify).

CPU tier: the big-int restatement (tests/ed25519_ref.py) against RFC 8032 TEST 1 and the three
real JoinSplit signatures of block 419221, every fixture status recomputed, the kernel's own
per-item routine compiled for the host (tests/native/zg_hosttest_ed25519.hip) bit-exact on every
fixture and on the two debug products, and the collector's error precedence with injected
verifiers.
GPU tier: zg_ed25519_verify against the fixture statuses (bit-exact verdict and error class), the
wave tail and second-block sizes, a 4,097-item batch with 1 % corrupted items, the field / scalar
debug products, and the collector through a real context."""
import ctypes
import os
import random
import shutil
import subprocess

import pytest

from tests import ed25519_ref as E
from tests.conftest import load_golden

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST_SRC = os.path.join(HERE, "native", "zg_hosttest_ed25519.hip")
HOST_LIB = os.path.join(HERE, "native", "libzg_hosttest_ed25519.so")
CSRC = os.path.join(ROOT, "zebra_amd", "csrc")

needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")

REAL_TX = {"53cf8971": "J2", "a2a2fe38": "J3", "70abe357": "J4"}   # tests/test_collector.py SRC_TX


def h(x):
    return bytes.fromhex(x)


_FIX = None


def fixture_items():
    """(name, pubkey, sig, msg, status) of real + signed + edges, computed once"""
    global _FIX
    if _FIX is None:
        g = load_golden("ed25519.json")
        out = [("real_" + e["txid"][:8], h(e["pubkey"]), h(e["sig"]), h(e["sighash"]), 0) for e in g["real"]]
        out += [("signed_%d" % i, h(e["pubkey"]), h(e["sig"]), h(e["msg"]), 0) for i, e in enumerate(g["signed"])]
        out += [(e["name"], h(e["pubkey"]), h(e["sig"]), h(e["msg"]), e["status"]) for e in g["edges"]]
        _FIX = out
    return _FIX


def run(ctx, items):
    return ctx.ed25519_verify([i[1] for i in items], [i[2] for i in items], [i[3] for i in items])


def field_pairs(field):
    """the operand pairs of the debug products (fields 5 and 6), shared by the host and the GPU test"""
    edge = [0, 1, E.P - 1, E.P, 2 ** 255 - 1, 2 ** 256 - 1, E.L - 1, E.L]
    rnd = random.Random(50 + field)
    return [(a, b) for a in edge for b in edge] + [(rnd.randrange(2 ** 256), rnd.randrange(2 ** 256))
                                                   for _ in range(256)]


def check_products(field, pairs, got):
    for (a, b), g in zip(pairs, got):
        want = a * b % E.P if field == 5 else (a + (b << 256)) % E.L
        assert int.from_bytes(g, "little") == want, (field, hex(a), hex(b))


# ------------------------------------------------------------------ CPU tier
def test_helper_rfc8032_and_real_signatures():
    g = load_golden("ed25519.json")
    t = g["rfc8032"][0]
    assert t == E.RFC8032_TEST1
    assert E.public_key(h(t["seed"])) == h(t["pubkey"])
    assert E.sign(h(t["seed"]), h(t["msg"])) == h(t["sig"])
    assert E.verify(h(t["pubkey"]), h(t["sig"]), h(t["msg"])) == E.OK
    assert len(g["real"]) == 3
    for e in g["real"]:
        assert E.verify(h(e["pubkey"]), h(e["sig"]), h(e["sighash"])) == E.OK, e["txid"]


def test_fixture_statuses_recomputed():
    items = fixture_items()
    assert len(items) == 3 + 48 + 16
    for name, pk, sg, m, st in items:
        assert E.verify(pk, sg, m) == st, name
    sts = [i[4] for i in items]
    assert all(sts.count(k) >= 2 for k in range(4))
    want = {"pk_not_on_curve": 1, "pk_bad_and_s_high": 1, "s_bit253": 2, "s_bit254": 2, "s_bit255": 2, "s_plus_l": 0,
            "msg_flip": 3, "r_flip": 3, "other_valid_key": 3, "a_identity_noncanonical": 0, "a_x0_signbit": 0,
            "a_order8": 0, "r_identity_ok": 0, "r_noncanonical": 3, "r_identity_signbit": 3}
    got = {i[0]: i[4] for i in items}
    for name, st in want.items():
        assert got[name] == st, name
    assert "all_zero" in got


_HOST = None


def host_lib():
    """the kernel's per-item routine and debug products compiled for the CPU (--offload-host-only),
    built on demand like tests/hostlib.py"""
    global _HOST
    if _HOST is None:
        deps = [HOST_SRC] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
        if not os.path.exists(HOST_LIB) or any(os.path.getmtime(d) > os.path.getmtime(HOST_LIB) for d in deps):
            subprocess.check_call(["hipcc", "-x", "hip", "--offload-host-only", "-O2", "-fPIC", "-shared",
                                   "-std=c++17", "-Wno-psabi", HOST_SRC, "-o", HOST_LIB])
        _HOST = ctypes.CDLL(HOST_LIB)
    return _HOST


@needs_hipcc
def test_host_compiled_kernel_routine_on_every_fixture():
    items = fixture_items()
    assert len(items) == 67
    st = ctypes.create_string_buffer(len(items))
    assert host_lib().zgt_ed25519_verify(ctypes.c_size_t(len(items)), b"".join(i[1] for i in items),
                                         b"".join(i[2] for i in items), b"".join(i[3] for i in items), st) == 0
    bad = [(i[0], i[4], g) for i, g in zip(items, st.raw) if g != i[4]]
    assert not bad, bad


@needs_hipcc
@pytest.mark.parametrize("field", [5, 6])
def test_host_compiled_field_products(field):
    pairs = field_pairs(field)
    out = ctypes.create_string_buffer(32 * len(pairs))
    host_lib().zgt_ed25519_field_mul(field, ctypes.c_size_t(len(pairs)),
                                     b"".join(a.to_bytes(32, "little") for a, _ in pairs),
                                     b"".join(b.to_bytes(32, "little") for _, b in pairs), out)
    check_products(field, pairs, [out.raw[32 * i:32 * i + 32] for i in range(len(pairs))])


def real_window():
    """three transactions carrying the real JoinSplits with their (pubkey, sig, sighash)"""
    from tests.test_collector import fields, make_tx
    F = fields()
    g = load_golden("ed25519.json")
    txs = []
    for e in g["real"]:
        tx = make_tx([REAL_TX[e["txid"][:8]]], F)
        assert tx.js_pubkey == h(e["pubkey"])
        tx.js_sig, tx.sighash = h(e["sig"]), h(e["sighash"])
        txs.append(tx)
    return txs


def fake_verify(bad=()):
    """a proof verifier that fails the proofs at the given window positions"""
    def verify(proofs, kinds, inputs, n_inputs):
        return [2 if i in bad else 0 for i in range(len(kinds))]
    return verify


def ref_js_sigs(pubkeys, sigs, msgs):
    return [E.verify(p, s, m) for p, s, m in zip(pubkeys, sigs, msgs)]


def test_collector_precedence_with_injected_verifiers():
    from zebra_amd import zg
    from zebra_amd.collector import verify_block
    calls = []

    def js(pubkeys, sigs, msgs):
        calls.append(len(pubkeys))
        return ref_js_sigs(pubkeys, sigs, msgs)

    assert verify_block(real_window(), verify=fake_verify(), verify_js_sigs=js) is None
    assert calls == [3]                                   # ONE call for the window
    for k in range(3):
        t = real_window()
        t[k].js_sig = t[k].js_sig[:7] + bytes([t[k].js_sig[7] ^ 1]) + t[k].js_sig[8:]
        # ... ahead of an InvalidJoinSplit on the same transaction (proof k fails too)
        assert verify_block(t, verify=fake_verify({k}), verify_js_sigs=js) == (k, "JoinSplitSignature")
        assert verify_block(real_window(), verify=fake_verify({k}), verify_js_sigs=js) == (k, ("InvalidJoinSplit", 0))
    # every non-zero status is the same error
    for st in (zg.ED_PUBLIC_ENCODING, zg.ED_SIGNATURE_ENCODING, zg.ED_SIGNATURE):
        assert verify_block(real_window(), verify=fake_verify(),
                            verify_js_sigs=lambda p, s, m, st=st: [0, st, 0]) == (1, "JoinSplitSignature")
    # a pre_error still wins
    t = real_window()
    t[1].js_sig = bytes(64)
    t[1].pre_error = "Eval"
    assert verify_block(t, verify=fake_verify(), verify_js_sigs=js) == (1, "Eval")
    # js_sig = None keeps js_sig_ok (and asks for no signature call)
    del calls[:]
    t = real_window()
    for tx in t:
        tx.js_sig = None
    assert verify_block(t, verify=fake_verify(), verify_js_sigs=js) is None
    t[2].js_sig_ok = False
    assert verify_block(t, verify=fake_verify(), verify_js_sigs=js) == (2, "JoinSplitSignature")
    assert calls == []
    # a carried signature overrides the caller's boolean
    t = real_window()
    t[0].js_sig_ok = False
    assert verify_block(t, verify=fake_verify(), verify_js_sigs=js) is None
    # js_sig without sighash raises; so does a carried signature without a backend
    t = real_window()
    t[1].sighash = None
    with pytest.raises(zg.ZgError):
        verify_block(t, verify=fake_verify(), verify_js_sigs=js)
    with pytest.raises(zg.ZgError):
        verify_block(real_window(), verify=fake_verify())


def corrupted_batch(n=4097, seed=5):
    """the fixtures' valid items cycled to n, 1 % corrupted in rotating ways -> (items, expected)"""
    valid = [i for i in fixture_items() if i[4] == 0 and not i[0].startswith(("a_", "r_", "s_"))]
    rnd = random.Random(seed)
    items = [list(valid[i % len(valid)]) for i in range(n)]
    want = [0] * n
    for c, i in enumerate(sorted(rnd.sample(range(n), n // 100))):
        _, pk, sg, m, _ = items[i]
        how = c % 5
        if how == 0:
            m = bytes([m[0] ^ (1 << rnd.randrange(8))]) + m[1:]
        elif how == 1:
            k = 32 + rnd.randrange(32)
            sg = sg[:k] + bytes([sg[k] ^ (1 + rnd.randrange(255))]) + sg[k + 1:]
        elif how == 2:
            k = rnd.randrange(256)
            sg = sg[:k // 8] + bytes([sg[k // 8] ^ (1 << (k % 8))]) + sg[k // 8 + 1:]
        elif how == 3:
            k = rnd.randrange(256)
            pk = pk[:k // 8] + bytes([pk[k // 8] ^ (1 << (k % 8))]) + pk[k // 8 + 1:]
        else:
            sg = sg[:32] + (int.from_bytes(sg[32:], "little") + E.L).to_bytes(32, "little")   # still valid
        items[i] = ["corrupt", pk, sg, m, None]
        want[i] = E.verify(pk, sg, m)
    return items, want


def test_corrupted_batch_expectation():
    """the 4,097-item batch of the GPU test: its non-zero count for the chosen seed, here on the CPU"""
    items, want = corrupted_batch()
    assert len(items) == 4097
    nz = sum(1 for s in want if s)
    assert 20 < nz < 70, nz


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
        batch[-1] = edges[k % len(edges)]   # a different non-zero edge case at the last index of each size
        got = run(ctx, batch)
        assert got == [b[4] for b in batch], n


@pytest.mark.gpu
def test_gpu_corrupted_batch(ctx):
    items, want = corrupted_batch()
    got = run(ctx, items)
    assert got == want, [(i, w, g) for i, (w, g) in enumerate(zip(want, got)) if w != g][:8]
    assert 20 < sum(1 for s in got if s) < 70


@pytest.mark.gpu
@pytest.mark.parametrize("field", [5, 6])
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
    assert verify_block(real_window(), ctx=c) is None
    for k in range(3):
        t = real_window()
        t[k].js_sig = t[k].js_sig[:40] + bytes([t[k].js_sig[40] ^ 0x10]) + t[k].js_sig[41:]
        assert verify_block(t, ctx=c) == (k, "JoinSplitSignature")
