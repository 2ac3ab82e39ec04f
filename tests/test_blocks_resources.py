"""Kernel resource guard of the block-body unit (CPU tier: hipcc cross-compiles gfx950, no GPU needed).
zg_blocks.hip is compiled with -Rpass-analysis=kernel-resource-usage (tools/resource_table.py) and the as-built
figures are held as ceilings: both kernels keep the hash state and the message block in registers (DESIGN.md
section 7i) -- no private segment, no spills, no LDS -- and k_txid stays within 128 VGPRs, so four waves per SIMD
fit: its read-ahead hides load latency only when there are other waves to switch to."""
import shutil
import tempfile

import pytest

from tools import resource_table

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")

# kernel -> (VGPR ceiling, scratch bytes per lane, LDS bytes, waves per SIMD at least): the figures of
# profiles/f12_resource_usage.txt
CEILINGS = {"k_txid": (96, 0, 0, 4), "k_block_merkle": (63, 0, 0, 4)}


def test_block_kernels_stay_in_registers():
    with tempfile.TemporaryDirectory() as tmp:
        rows = {r["name"]: r for r in resource_table.unit("zg_blocks.hip", tmp) if "occ" in r}
    assert len(rows) == len(CEILINGS), sorted(rows)
    for part, (vgpr, scratch, lds, occ) in CEILINGS.items():
        (name, r), = [(n, r) for n, r in rows.items() if part in n]
        assert r["vgpr"] <= vgpr <= 128 and r["scratch"] <= scratch and r["lds"] <= lds, (name, r)
        assert r.get("vspill", 0) == 0 and r.get("sspill", 0) == 0 and r["occ"] >= occ, (name, r)
