#!/usr/bin/env python3
"""Writes tests/golden/ref_tables.npz: the numbers the reference holds as table data (circShift_* and posBnInCnProcBuf_*
of nrLDPC_lut.h, the group populations of nrLDPCdecoder_defs.h, index_k0 of nr_rate_matching.c), read by
tests/test_tables.py:reference_table_data().  Needs the reference tree; the fixture is DATA, one int32 array per table.

  python tools/make_ref_table_fixtures.py
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import test_tables as T  # noqa: E402

data = T.reference_table_data()
np.savez_compressed(ROOT / "tests" / "golden" / "ref_tables.npz", **data)
print(f"{len(data)} arrays, {sum(v.size for v in data.values())} numbers")
