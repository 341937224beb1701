"""Records tests/golden/out_files_sha256.json: length and SHA-256 of every file of tests/out_files.py as the
library of the checked-out commit writes them on an MI355X.  Run from a checkout of the commit whose files are to be
the reference, with the library built:

usage: python tests/golden/out_files_golden.py <commit id>
"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "ucla-roms_amd"))

import out_files  # noqa: E402


def main(commit):
    with tempfile.TemporaryDirectory() as d:
        files = out_files.write_all(d)
    doc = {"header": "files of tests/out_files.py as written by commit %s" % commit,
           "files": {k: {"bytes": v[0], "sha256": v[1]} for k, v in files.items()}}
    with open(os.path.join(HERE, "out_files_sha256.json"), "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(doc, indent=1, sort_keys=True))


if __name__ == "__main__":
    main(sys.argv[1])
