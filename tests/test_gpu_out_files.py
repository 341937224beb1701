"""Every kind of file the library writes is, byte for byte, what the commit named in
tests/golden/out_files_sha256.json wrote for the same run (tests/out_files.py)."""
import json
import os

import pytest

import out_files

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def test_every_file_is_the_recorded_one(tmp_path):
    want = json.load(open(os.path.join(HERE, "golden", "out_files_sha256.json")))["files"]
    got = out_files.write_all(tmp_path)
    assert sorted(got) == sorted(want) and len(want) == 9
    for name, w in want.items():
        assert got[name] == (w["bytes"], w["sha256"]), name
