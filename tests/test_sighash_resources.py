"""Kernel resource guard of the signature-hash unit (CPU tier: hipcc cross-compiles gfx950, no GPU needed).
zg_sighash.hip is compiled with -Rpass-analysis=kernel-resource-usage (tools/resource_table.py) and the
as-built figures are held as ceilings: both kernels keep the hash state and the 16-word message block in
registers (the word funnel) -- no private segment, no LDS, two waves per SIMD."""
import shutil
import tempfile

import pytest

from tools import resource_table

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")

# kernel -> (VGPR ceiling, scratch bytes per lane, LDS bytes): the figures of profiles/f10_sighash_resource_usage.txt
CEILINGS = {"k_sighash_digests": (199, 0, 0), "k_sighash_items": (242, 0, 0)}


def test_sighash_kernels_stay_in_registers():
    with tempfile.TemporaryDirectory() as tmp:
        rows = {r["name"]: r for r in resource_table.unit("zg_sighash.hip", tmp) if "occ" in r}
    assert len(rows) == len(CEILINGS), sorted(rows)
    for part, (vgpr, scratch, lds) in CEILINGS.items():
        (name, r), = [(n, r) for n, r in rows.items() if part in n]
        assert r["vgpr"] <= vgpr and r["scratch"] <= scratch and r["lds"] <= lds, (name, r)
        assert r.get("vspill", 0) == 0 and r.get("sspill", 0) == 0 and r["occ"] >= 2, (name, r)
