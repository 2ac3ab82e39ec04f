"""GPU tier of the signature-kernel edge tests: the vectors of tests/sig_edges.py (read its docstring;
tests/test_sig_edges.py pins them against the references) through Context.redjubjub_verify, sapling_bvk,
jubjub_decode, ed25519_verify and ecdsa_verify.

Every reachable entry of the device-built comb tables of k_jj_comb (three generators), k_ed_comb and
k_ec_comb is read by exactly one accepted item, so a wrong entry is one wrong verdict and the failure
names (table, w, d); every window also has a twin that must be rejected. Each kernel's set goes in
one call in a seeded shuffled order, of a size that is no whole number of waves. The RedJubjub items that
only the cofactor accepts fail the day k_redjubjub loses its three doublings."""
import ctypes

import pytest

from tests import sig_edges as E

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from zebra_amd import Context
    c = Context(device=0, max_batch=64, load_builtin=False)
    yield c
    c.close()


def _rj(ctx, items):
    got = ctx.redjubjub_verify([i.vk for i in items], [i.sig for i in items], [i.msg for i in items],
                               [i.gen for i in items])
    bad = [(i.name, "want %s" % i.ok) for i, g in zip(items, got) if g != i.ok]
    assert not bad, (len(bad), bad[:8])
    assert len(got) == len(items)


def _statuses(got, items):
    bad = [(i.name, "want %d got %d" % (i.status, g)) for i, g in zip(items, got) if g != i.status]
    assert not bad, (len(bad), bad[:8])
    assert len(got) == len(items)


def _bvk(ctx, rows):
    got = ctx.sapling_bvk([(list(r.spends), list(r.outputs), r.value) for r in rows])
    bad = [(n, r.name, "want %d %s got %d %s" % (r.status, r.bvk.hex(), st, key.hex()))
           for n, (r, (st, key)) in enumerate(zip(rows, got)) if (st, key) != (r.status, r.bvk)]
    assert not bad, (len(bad), bad[:4])
    assert len(got) == len(rows)


# ----------------------------------------------------------------------------- A. the comb tables
def test_redjubjub_every_reachable_table_entry(ctx):
    entries, twins = E.redjubjub_table_items()
    assert len(entries) == 2 * 7919 and len(twins) == 64
    _rj(ctx, E.shuffled(entries + twins, 0x51))


def test_value_balance_every_reachable_table_entry(ctx):
    rows = E.gv_table_rows()
    assert len(rows) == 2 * 1912
    _bvk(ctx, E.shuffled(rows, 0x52))


def test_ed25519_every_reachable_table_entry(ctx):
    entries, twins, unreadable = E.ed25519_table_items()
    assert len(entries) == 7936 and len(twins) == 32 and len(unreadable) == 224
    items = E.shuffled(entries + twins, 0x53)
    _statuses(ctx.ed25519_verify([i.pubkey for i in items], [i.sig for i in items], [i.msg for i in items]), items)
    # the S that would read the other 224 entries never gets that far
    _statuses(ctx.ed25519_verify([i.pubkey for i in unreadable], [i.sig for i in unreadable],
                                 [i.msg for i in unreadable]), unreadable)


def test_ecdsa_every_table_entry(ctx):
    entries, twins = E.ecdsa_table_items()
    assert len(entries) == 8160 and len(twins) == 64
    items = E.shuffled(entries + twins, 0x54)
    _statuses(ctx.ecdsa_verify([i.pubkey for i in items], [i.sig for i in items], [i.msg for i in items]), items)


# ----------------------------------------------------------------------------- B. RedJubjub named items
def test_redjubjub_cofactor_and_boundary_items(ctx):
    items = E.redjubjub_named_items()
    assert sum(i.name.startswith("torsion") for i in items) == 12
    _rj(ctx, items)


def test_redjubjub_gen_byte_selects_binding_or_spend_auth(ctx):
    """include/zg.h: ZG_GEN_BINDING is the binding generator, every other byte the spend-auth one"""
    _rj(ctx, E.redjubjub_gen_byte_items())


def test_redjubjub_sizes_wave_tail_and_second_block(ctx):
    batches = E.redjubjub_size_batches()
    assert [len(b) for b in batches] == [0, 1, 1, 63, 64, 65, 129]
    assert ctx.redjubjub_verify([], [], [], []) == []
    for b in batches[1:]:
        _rj(ctx, b)


# ----------------------------------------------------------------------------- C. bvk rows, decode points
def test_bvk_ragged_rows_with_failing_neighbours(ctx):
    batches = E.bvk_batches()
    assert [len(b) for b in batches] == list(E.SIZES)
    assert ctx.sapling_bvk([]) == []
    for rows in batches:
        _bvk(ctx, rows)
    _bvk(ctx, [batches[-1][11]])            # one good row alone (the one-row batch above is a failing row)
    _bvk(ctx, [batches[-1][3]])             # no cvs at all in the call: the identity encoding


def test_jubjub_decode_torsion_and_field_ends(ctx):
    from zebra_amd.zg import lib
    assert ctx.jubjub_decode([]) == []
    for pts, want in E.decode_batches():
        got = ctx.jubjub_decode(pts)
        bad = [(p.hex(), w, g) for p, w, g in zip(pts, want, got) if w != g]
        assert not bad and len(got) == len(pts), bad[:4]
        # xy = NULL: the statuses alone (the wrapper always passes a buffer, so the ABI directly)
        n = len(pts)
        st = ctypes.create_string_buffer(b"\xee" * n, n)
        assert lib().zg_jubjub_decode(ctx._p, n, b"".join(pts), st, None) == 0
        assert list(st.raw) == [w[0] for w in want]
