#!/usr/bin/env python3
"""Writes tests/golden/ref_abi_layouts.json: the sizes, offsets and enum values the reference's own headers give the plugin
ABI structures (tests/test_abi.py:reference_layouts, compiled against the reference tree), read by
test_layouts_against_the_reference_headers.  Needs the reference tree; the fixture is DATA (printed numbers, field names).

  python tools/make_ref_abi_fixture.py
"""
import json
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import test_abi as T  # noqa: E402

with tempfile.TemporaryDirectory() as d:
    data = T.reference_layouts(Path(d))
(ROOT / "tests" / "golden" / "ref_abi_layouts.json").write_text(json.dumps(data, indent=1) + "\n")
print(len(data["enc_fields"]), "encoder fields,", data["abi_offsets"].count("\n"), "layout lines")
