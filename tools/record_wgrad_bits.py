"""Writes tests/golden/wgrad_x3_bits.json: per key of tests/wgrad_bits_cases.py the SHA-256 of dW's bytes on THIS tree.  Run it on the
MI355X on the commit whose weight-gradient kernels are the reference, and commit the file; tests/test_gpu_wgrad_bits.py then holds
later trees to it.  Every key is run twice in the process, and no file is written if the two hashes of any key differ.
python tools/record_wgrad_bits.py <commit the tree is at> [output path]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import wgrad_bits_cases as wb  # noqa: E402


def main(argv):
    if len(argv) < 2:
        raise SystemExit(__doc__)
    path = argv[2] if len(argv) > 2 else os.path.join(ROOT, "tests", "golden", "wgrad_x3_bits.json")
    first = {key: wb.digest(key) for key in wb.KEYS}
    second = {key: wb.digest(key) for key in wb.KEYS}
    differ = [key for key in wb.KEYS if first[key] != second[key]]
    if differ:
        raise SystemExit("not written: two runs of the same tree differ in %s" % differ)
    with open(path, "w") as f:
        f.write('{"recorded_at": %s, "sha256": {\n' % json.dumps(argv[1]))
        f.write(",\n".join(" %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in first.items()))
        f.write("\n}}\n")
    print("%s: %d keys, each run twice with equal hashes" % (path, len(first)))


if __name__ == "__main__":
    main(sys.argv)
