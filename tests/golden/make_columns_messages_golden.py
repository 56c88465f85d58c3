#!/usr/bin/env python3
"""Writes tests/golden/columns_messages_golden.json: name -> [return code, exact text of dsrcgpu_last_error] for every case of
tests/columns_messages_cases.py, taken from the emulator build of the library (tests/emu/libdsrc_emu.so; the host code is the same in
both builds).

The file on record was made from the commit BEFORE the columnar host layer moved into dsrc_amd/csrc/host_columns.h, so that the
rewrite is held to the old wording.  Do not run this to make a failing test pass: a message that changes is a change of the
library's behaviour and is decided as one.  Run it only to ADD cases, on a tree whose existing cases pass, and check that the diff
of the JSON has additions only."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "emu")], stdout=subprocess.DEVNULL)
os.environ["DSRC_GPU_LIB"] = os.path.join(ROOT, "tests", "emu", "libdsrc_emu.so")

from dsrc_amd import _lib  # noqa: E402
from tests import columns_messages_cases as cases  # noqa: E402

got = cases.collect(_lib)
with open(cases.GOLDEN, "w") as f:
    json.dump(got, f, indent=1, sort_keys=True)
    f.write("\n")
print(len(got), "cases,", sum(1 for v in got.values() if v[0]), "refused")
