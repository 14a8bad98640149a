"""Writes a golden file of output hashes: per key of a cases module under tests/ the SHA-256 its digest(key) gives on THIS tree —
tests/golden/wgrad_x3_bits.json for wgrad_bits_cases (dW's bytes; the default), tests/golden/pw_x3_bits.json for pw_bits_cases (the
output buffers of csrc/pw_x3.hip's entries).  Run it on the MI355X on the commit whose kernels are the reference, and commit the file;
tests/test_gpu_wgrad_bits.py / tests/test_gpu_pw_bits.py then hold later trees to it.  Every key is run twice in the process, and no
file is written if the two hashes of any key differ.
python tools/record_wgrad_bits.py <commit the tree is at> [cases module [output path]]"""
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

GOLDEN = {"wgrad_bits_cases": "wgrad_x3_bits.json", "pw_bits_cases": "pw_x3_bits.json"}


def main(argv):
    if len(argv) < 2:
        raise SystemExit(__doc__)
    module = argv[2] if len(argv) > 2 else "wgrad_bits_cases"
    wb = importlib.import_module(module)
    path = argv[3] if len(argv) > 3 else os.path.join(ROOT, "tests", "golden", GOLDEN[module])
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
