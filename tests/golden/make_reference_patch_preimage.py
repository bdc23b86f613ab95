"""Generates tests/golden/reference_patch_preimage.json from a checkout of the reference: for every file integration/reference.patch
touches, the file's line count and, for every hunk, the SHA-256 of the lines the reference has where the hunk applies.  No source text
is stored.  tests/test_abi.py::test_reference_patch_applies checks the patch against it without the reference at hand:

    python tests/golden/make_reference_patch_preimage.py <reference checkout>
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_abi import PATCH, PATCH_PREIMAGE, parse_patch  # noqa: E402

ref = sys.argv[1]
out = {"what": "per file of integration/reference.patch: the reference's line count and, per hunk, the SHA-256 of its lines "
               "[start, start + count) with their newlines (tests/golden/make_reference_patch_preimage.py)", "files": {}}
for f, hunks in parse_patch(PATCH).items():
    lines = open(os.path.join(ref, f), "rb").read().split(b"\n")
    lines = [l + b"\n" for l in lines[:-1]] + ([lines[-1]] if lines[-1] else [])
    out["files"][f] = {"lines": len(lines), "hunks": [{"start": s, "count": n, "sha256": hashlib.sha256(b"".join(lines[s - 1:s - 1 + n])).hexdigest()}
                                                      for s, n, *_ in hunks]}
json.dump(out, open(PATCH_PREIMAGE, "w"), indent=1, sort_keys=True)
print(f"wrote {os.path.relpath(PATCH_PREIMAGE, ROOT)}: {sum(len(v['hunks']) for v in out['files'].values())} hunks in {len(out['files'])} files")
