#!/usr/bin/env python3
"""Record what the tests need to know about the reference tree, as digests, so that they run without it.

Writes tests/golden/reference_snapshot.json:
  files      for every reference file the tests derive something from -- the files integration/0001-*.patch modifies and
             pkg/lwepp/handlers/request_test.go (the source of reference_cases.json) -- its sha256 and line count, and for
             every hunk of the patch on it [old_start, old_len, sha256 of the reference's lines old_start .. old_start + old_len - 1];
  absent     the files the patch creates that the reference does not have;
  contains   whether a reference file holds each string of NEEDLES.
No source text is stored: only digests, counts and yes / no answers.

Run with the root of a reference checkout as the argument:
    python tests/golden/extract_reference_snapshot.py <reference checkout>
tests/test_integration_patch.py and tests/test_reference_cases.py read the committed JSON.
"""
from __future__ import annotations

import hashlib
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PATCH = os.path.join(ROOT, "integration", "0001-lwepp-gpu-endpoint-picker.patch")
OUT = os.path.join(HERE, "reference_snapshot.json")
CASES_SOURCE = "pkg/lwepp/handlers/request_test.go"
NEEDLES = {"pkg/lwepp/handlers/server.go": ["func NewStreamingServer(datastore Datastore) *StreamingServer"],
           "pkg/lwepp/handlers/request_test.go": ["NewStreamingServer(ds)"]}

HUNK_RE = re.compile(r"^@@ -(\d+)(?:,(\d+))? \+(\d+)(?:,(\d+))? @@")


def patch_hunks(text: str):
    """({path: [(old_start, old_len, body lines)]} of the files a unified diff modifies, [paths of the files it creates])."""
    modified, created = {}, []
    lines = text.splitlines()
    i = 0
    while i < len(lines):
        if not (lines[i].startswith("--- ") and i + 1 < len(lines) and lines[i + 1].startswith("+++ ")):
            i += 1
            continue
        old = lines[i][4:].split("\t")[0]
        path = lines[i + 1][4:].split("\t")[0].split("/", 1)[1]
        hunks = []
        i += 2
        while i < len(lines) and lines[i].startswith("@@"):
            m = HUNK_RE.match(lines[i])
            a, b = int(m.group(1)), int(m.group(2) or 1)
            n_old, n_new = b, int(m.group(4) or 1)
            body = []
            i += 1
            while n_old or n_new:
                ln = lines[i]
                if not ln.startswith("\\"):
                    body.append(ln)
                    n_old -= ln[:1] in (" ", "-")
                    n_new -= ln[:1] in (" ", "+")
                i += 1
            hunks.append((a, b, body))
        if old == "/dev/null" or all(a == 0 and b == 0 for a, b, _ in hunks):
            created.append(path)
        else:
            modified[path] = hunks
    return modified, created


def digest_lines(lines) -> str:
    return hashlib.sha256(("\n".join(lines) + "\n").encode()).hexdigest()


def preimage(body):
    """The lines a hunk expects in the original file: its context and removed lines, in order."""
    return [ln[1:] for ln in body if ln[:1] in (" ", "-")]


def main() -> int:
    if len(sys.argv) != 2 or not os.path.isdir(sys.argv[1]):
        print(__doc__)
        return 2
    ref = sys.argv[1]
    modified, created = patch_hunks(open(PATCH).read())
    files = {}
    for path in sorted(set(modified) | {CASES_SOURCE}):
        raw = open(os.path.join(ref, path), "rb").read()
        lines = raw.decode().splitlines()
        files[path] = {"sha256": hashlib.sha256(raw).hexdigest(), "lines": len(lines),
                       "hunks": [[a, b, digest_lines(lines[a - 1:a - 1 + b])] for a, b, _ in modified.get(path, [])]}
    doc = {
        "generated_by": "tests/golden/extract_reference_snapshot.py",
        "files": files,
        "absent": sorted(p for p in created if not os.path.exists(os.path.join(ref, p))),
        "contains": {p: {s: s in open(os.path.join(ref, p)).read() for s in ss} for p, ss in NEEDLES.items()},
    }
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(files)} reference files, {sum(len(v['hunks']) for v in files.values())} hunks -> {OUT}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
