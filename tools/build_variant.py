#!/usr/bin/env python3
"""A/B tooling: link zebra_amd/libzg_<name>.so from the in-tree objects, with the listed units
recompiled under extra -D switches (loaded by ZG_LIB_VARIANT=<name>, zebra_amd/zg.py).
Usage: python tools/build_variant.py NAME UNIT.hip[,UNIT.hip] -DFOO=1 [-DBAR=0 ...]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from zebra_amd import build as zb  # noqa: E402


def main():
    name, units, defs = sys.argv[1], sys.argv[2].split(","), sys.argv[3:]
    print(zb.build_variant(name, units, defs))


if __name__ == "__main__":
    main()
