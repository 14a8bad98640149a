"""Writes tests/golden/pw_x3_domain.json: what csrc/pw_x3.hip's `*_supported` / `*_rows` queries answer on THIS tree's library, as
tests/test_pw_domain_host.py summarises them (one SHA-256 and the count of supported points per entry).  No device is needed.  Run it
on the commit whose domain is the reference, and commit the file.
python tools/record_pw_domain.py <commit the tree is at> [output path]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_pw_domain_host as dom  # noqa: E402


def main(argv):
    if len(argv) < 2:
        raise SystemExit(__doc__)
    path = argv[2] if len(argv) > 2 else dom.GOLDEN
    entries = dom.summary()
    with open(path, "w") as f:
        f.write('{"recorded_at": %s, "entries": {\n' % json.dumps(argv[1]))
        f.write(",\n".join(" %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in entries.items()))
        f.write("\n}}\n")
    print("%s: %s" % (path, {k: v["supported"] for k, v in entries.items()}))


if __name__ == "__main__":
    main(sys.argv)
