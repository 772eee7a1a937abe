#!/usr/bin/env python3
"""Record the scan of the reference's src/ directory that tests/test_julia_binding.py holds sites.json against:
tests/golden/reference_sites.json lists every site (file, line, a hash of the line's text) and the hash of each scanned file.
Run from the repo root with the reference's src/ directory:  python tests/golden/make_reference_sites.py PATH/TO/WaterLily.jl/src
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from test_julia_binding import PAT, REF_FILES, REF_SITES, SITES, scan_reference  # noqa: E402


def main(src):
    scope = json.load(open(SITES, encoding="utf-8"))["scope"]
    files = {f: hashlib.sha256(open(os.path.join(src, f), "rb").read()).hexdigest() for f in REF_FILES}
    rec = {"what": "scan of the reference's src/ by tests/test_julia_binding.py: scan_reference (text hash = sha256 of the stripped line's first 110 characters, 16 hex digits)",
           "pattern": PAT.pattern, "scope": scope, "files_sha256": files, "sites": scan_reference(src, scope)}
    head = ",\n".join(f"{json.dumps(k)}: {json.dumps(v, ensure_ascii=False)}" for k, v in rec.items() if k != "sites")
    body = ",\n".join(json.dumps(s) for s in rec["sites"])
    with open(REF_SITES, "w", encoding="utf-8") as fh:
        fh.write("{\n" + head + ',\n"sites": [\n' + body + "\n]}\n")
    print(f"{len(rec['sites'])} sites -> {REF_SITES}")


if __name__ == "__main__":
    main(sys.argv[1])
