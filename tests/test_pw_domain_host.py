"""The domain of csrc/pw_x3.hip's entries — what the five `*_supported` / `*_rows` queries answer — is the one
tests/golden/pw_x3_domain.json names (written by tools/record_pw_domain.py on the commit it records): per entry the SHA-256 over the
answers on a fixed grid, in a fixed order, and the number of supported points, so a mismatch says which entry moved.  The queries
need no device."""
import hashlib
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pw_x3_domain.json")
KS, NS = range(8, 1025, 8), range(16, 4097, 16)
ROWS_AT = ((96, 1), (4112, 1), (8224, 2), (100, 3))  # (m, groups) of the two *_rows entries


def answers():
    """{entry: [answer, ...]} over the grid, every list in the order of its loops."""
    from avtex import _lib
    L = _lib.lib()
    kn = [(k, n) for k in KS for n in NS]
    return {
        "avt_pw_x3_supported": [L.avt_pw_x3_supported(k, n) for k, n in kn],
        "avt_pw_x3_f32_supported": [L.avt_pw_x3_f32_supported(k, n) for k, n in kn],
        "avt_pw_x3_f32_stat_rows": [L.avt_pw_x3_f32_stat_rows(k, n, m, g) for k, n in kn for m, g in ROWS_AT],
        "avt_pw_x3_f32_bwdstats_rows": [L.avt_pw_x3_f32_bwdstats_rows(k, n, m, g) for k, n in kn for m, g in ROWS_AT],
        "avt_lateral_x3_supported": [L.avt_lateral_x3_supported(cin, cout, kt)
                                     for cin in range(8, 129, 8) for cout in range(8, 257, 8) for kt in range(1, 10)],
        "avt_pw_chain_x3_supported": [L.avt_pw_chain_x3_supported(k1, n1, n2)
                                      for k1 in (32, 64, 128) for n1 in (128, 256, 512) for n2 in (32, 64, 128)],
    }


def summary():
    """{entry: {"sha256": of the answers as little-endian int32, "supported": how many are > 0}}"""
    out = {}
    for name, vals in answers().items():
        a = np.asarray(vals, dtype="<i4")
        out[name] = {"sha256": hashlib.sha256(a.tobytes()).hexdigest(), "supported": int((a > 0).sum())}
    return out


def test_the_domain_is_the_recorded_one():
    with open(GOLDEN) as f:
        golden = json.load(f)["entries"]
    got = summary()
    assert list(got) == list(golden)
    moved = {name: (got[name]["supported"], golden[name]["supported"]) for name in got if got[name] != golden[name]}
    assert not moved, "entries whose answers moved (supported points now, recorded): %s" % moved
