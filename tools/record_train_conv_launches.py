"""Writes tests/golden/train_conv_launch_plan.json: what every case of tests/train_conv_cases.py sends to the C ABI (entry names, scalar
arguments, which pointers are null) on THIS tree.  Run it on the MI355X on the commit whose dispatch is the reference, and commit the
file; tests/test_gpu_train_conv_plan.py then holds later trees to it.
python tools/record_train_conv_launches.py <commit the tree is at> [output path]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import train_conv_cases as tc  # noqa: E402


def dumps(commit, plans):
    """One launch per line (a reviewable diff), keys in the case list's order."""
    out = ['{"recorded_at": %s, "cases": {' % json.dumps(commit)]
    for i, (case, plan) in enumerate(plans.items()):
        out.append(' %s: {' % json.dumps(case))
        for j, (key, calls) in enumerate(plan.items()):
            out.append('  %s: [' % json.dumps(key))
            out.extend('   %s%s' % (json.dumps(c), "," if n + 1 < len(calls) else "") for n, c in enumerate(calls))
            out.append('  ]%s' % ("," if j + 1 < len(plan) else ""))
        out.append(' }%s' % ("," if i + 1 < len(plans) else ""))
    out.append('}}')
    return "\n".join(out) + "\n"


def main(argv):
    if len(argv) < 2:
        raise SystemExit(__doc__)
    path = argv[2] if len(argv) > 2 else os.path.join(ROOT, "tests", "golden", "train_conv_launch_plan.json")
    plans = {case: tc.plan(case) for case in tc.CASES}
    text = dumps(argv[1], plans)
    assert json.loads(text)["cases"] == json.loads(json.dumps(plans))
    with open(path, "w") as f:
        f.write(text)
    print("%s: %d cases, %d launches" % (path, len(plans), sum(len(c) for p in plans.values() for c in p.values())))


if __name__ == "__main__":
    main(sys.argv)
