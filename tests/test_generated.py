"""CPU tier: every generated header under zebra_amd/csrc is what its generator writes today, byte
for byte, so an edit to a generator (or to a header by hand) cannot drift unnoticed. Each
generator runs as its docstring says: a child process whose stdout is the header."""
import os
import subprocess
import sys

import pytest

from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "zebra_amd", "csrc")
GENERATED = [("gen_constants.py", "zg_constants.h"), ("gen_fips.py", "zg_fips.h"), ("gen_fq29.py", "zg_fq29_gen.h"),
             ("gen_coop.py", "zg_coop_tables.h"), ("gen_prog.py", "zg_prog_tables.h")]


@pytest.mark.parametrize("gen,header", GENERATED, ids=[h for _, h in GENERATED])
def test_generator_reproduces_header(gen, header):
    r = subprocess.run([sys.executable, os.path.join(CSRC, gen)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    with open(os.path.join(CSRC, header), "rb") as f:
        want = f.read()
    assert r.stdout == want, "%s no longer writes the committed %s" % (gen, header)
