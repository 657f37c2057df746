#!/usr/bin/env python3
"""Run bench.py against an experiment build of the library: tools/bench_with_lib.py <lib.so> [bench.py args...]
(a build of THIS tree's ABI and exports; a parent commit's library is measured with that commit's own tree and bench.py)"""
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
lib = os.path.abspath(sys.argv[1])
sys.argv = ["bench.py"] + sys.argv[2:]
import tsxform
tsxform._native.LIB_PATH = lib
tsxform._native.Native.__init__.__defaults__ = (lib,)    # bench.py calls Native(): the default was bound to the package's library at import
import bench
bench.main()
