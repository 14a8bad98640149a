"""Plain restatements of the plane makers of csrc/stem_train.hip (test infrastructure, never imported by the product, and calling
nothing of the package or of oracle/): the row-scaled fp16 / plain bf16 weight planes, the transposed and tap-selected planes of the
input gradient's filter, the gathered rows of the pixel-grouped layers and the clip's pixel planes — numpy, one float32 operation per
operation of the kernel, on top of split / join of tests/pack_pool_refs.py (split2 word for word).  And the EDGE INPUTS, as functions,
so that tests/test_weight_planes_refs_host.py (CPU) and tests/test_gpu_weight_planes_edges.py (device) see the same arrays.

The contract the host test holds these (and the package's torch route) to, against float64:
  fp16 planes  |w - (hi + lo) * wscale| <= max(2^-22 |w|, 2^-25 wscale) per finite element — two round-to-nearest fp16 steps on the
               scaled value, the second a denormal (step 2^-24) when the remainder is below 2^-14 — and the row's largest finite
               magnitude, divided by wscale, in [2^9, 2^10) for every row whose maximum is at least 1e-30;
  bf16 planes  |w - (hi + lo)| <= max(2^-16 |w|, 2^-134) for |w| <= BF16_TOP (csrc/split_planes.h: below 2^-126 the low plane is a
               bf16 denormal of step 2^-133; above BF16_TOP the high plane rounds to an infinity)."""
import numpy as np

from pack_pool_refs import BF16, F16, F32, join, plane_f32, plane_tensor, split, words  # noqa: F401  (re-exported for the tests)

FLT_MAX = np.finfo(np.float32).max
BF16_TOP = np.array([0x7F7F7FFF], np.uint32).view(F32)[0]  # the largest fp32 that round-to-nearest-even keeps a FINITE bf16
NAN, INF = F32(np.nan), F32(np.inf)
SCALE_KS = (-100, -30, -1, 0, 1, 9, 10, 64, 127)
ROW_KS = (2, 4, 510, 512, 514, 1026)  # the split loop strides by 512 elements, the maximum loop by 256


# ---------------------------------------------------------------- the references
def finite_max(w):
    """Per row: the largest |entry| among the finite ones (0 when there is none)."""
    a = np.abs(np.asarray(w, F32))
    return np.where(np.isfinite(a), a, F32(0)).max(axis=-1)


def row_scale(w):
    """fp32 [rows, K] -> (sc, wscale) fp32 [rows]: mx = max(|finite entries|, 1e-30f), (m, e) = frexp(mx), sc = 2^(10 - e),
    wscale = 2^(e - 10).  mx * sc = m * 2^10 lies in [2^9, 2^10)."""
    mx = np.maximum(finite_max(w), F32(1e-30))
    _, e = np.frexp(mx)
    e = e.astype(np.int64)
    return np.ldexp(F32(1), 10 - e).astype(F32), np.ldexp(F32(1), e - 10).astype(F32)


def rows_ref(w, plane):
    """fp32 [rows, K] -> (hi, lo uint16 [rows, K], wscale fp32 [rows] | None).  fp16 planes: the split of fp32(row * sc); bf16 planes:
    the split of the row itself, no scale."""
    w = np.ascontiguousarray(w, dtype=F32)
    if plane == BF16:
        return split(w, BF16) + (None,)
    sc, wscale = row_scale(w)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        v = (w * sc[:, None]).astype(F32)
    return split(v, F16) + (wscale,)


def transposed_ref(w, sel):
    """fp32 [cout, taps, cin], sel -> bf16 planes (hi, lo) uint16 [cin, nsel, cout]: out[ci][a][co] = w[co][sel[a]][ci]."""
    w = np.asarray(w, F32)
    return split(np.ascontiguousarray(w[:, np.asarray(sel, np.int64), :].transpose(2, 1, 0)), BF16)


def gather_ref(storage, idx_map, plane):
    """storage fp32 [n] (a weight's memory), idx_map int32 [rows, K] -> rows_ref of the rows storage[idx_map], 0 where the map is -1."""
    s, m = np.asarray(storage, F32).reshape(-1), np.asarray(idx_map, np.int64)
    return rows_ref(np.where(m >= 0, s[np.maximum(m, 0)], F32(0)).astype(F32), plane)


def clip_ref(x, plane):
    """fp32 [B, 3, T, H, W] -> (hi, lo) uint16 [B, T, H, W, 4]: channels 0..2 the split of the pixel, channel 3 the split of 0."""
    x = np.asarray(x, F32)
    v = np.zeros((x.shape[0],) + x.shape[2:] + (4,), F32)
    v[..., :3] = np.moveaxis(x, 1, -1)
    return split(v, plane)


def is_nan_words(wd, plane):
    wd = np.asarray(wd, np.uint16)
    return ((wd & 0x7C00) == 0x7C00) & ((wd & 0x03FF) != 0) if plane == F16 else ((wd & 0x7F80) == 0x7F80) & ((wd & 0x007F) != 0)


def same_words(got, want, plane):
    """Plane words compared bit for bit; a NaN by kind (NaN against NaN), not payload.  -> bool array."""
    got, want = np.asarray(got, np.uint16), np.asarray(want, np.uint16)
    return (got == want) | (is_nan_words(got, plane) & is_nan_words(want, plane))


def bits32(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def scaled_back(hi, lo, wscale, plane):
    """float64 (hi + lo) * wscale (wscale None: 1): what a convolution's accumulator sees of the weight."""
    with np.errstate(invalid="ignore", over="ignore"):
        v = plane_f32(hi, plane).astype(np.float64) + plane_f32(lo, plane).astype(np.float64)
        return v if wscale is None else v * np.asarray(wscale, np.float64)[:, None]


def contract_ratio(w, hi, lo, wscale, plane):
    """-> (worst error / bound over the finite elements the bound speaks of, the rows' scaled maxima or None).  fp16 planes: every
    finite element; bf16 planes: |w| <= BF16_TOP."""
    w64 = np.asarray(w, F32).astype(np.float64)
    got = scaled_back(hi, lo, wscale, plane)
    if plane == F16:
        ws = np.asarray(wscale, np.float64)[:, None]
        bound, ok = np.maximum(2.0 ** -22 * np.abs(w64), 2.0 ** -25 * ws), np.isfinite(w64)
        scaled = finite_max(w).astype(np.float64) / ws[:, 0]
    else:
        bound, ok = np.maximum(2.0 ** -16 * np.abs(w64), 2.0 ** -134), np.isfinite(w64) & (np.abs(w64) <= float(BF16_TOP))
        scaled = None
    with np.errstate(invalid="ignore"):
        err = np.where(ok, np.abs(w64 - got), 0.0)
    assert np.isfinite(err).all(), "a finite weight came back as an infinity or a NaN"
    return float((err / np.where(ok, bound, 1.0)).max()), scaled


# ---------------------------------------------------------------- the edge inputs
def _rng(*key):
    return np.random.default_rng([int(k) & 0xFFFFFFFF for k in key] + [20251])


def _ulps(x, d):
    """fp32 x moved by d units in the last place (away from zero for d > 0)."""
    return (np.array([x], F32).view(np.uint32) + np.uint32(d & 0xFFFFFFFF)).view(F32)[0]


def scale_edge_maxima():
    """The maxima at which the scale's exponent steps: 2^k and one ulp either side for k in SCALE_KS, and FLT_MAX."""
    out = []
    for k in SCALE_KS:
        p = F32(2.0) ** F32(k)
        out += [_ulps(p, -1), p, _ulps(p, 1)]
    return out + [FLT_MAX]


def _row(K, mx, pos, key, rel=0.97, sign=1.0):
    """A row whose largest magnitude is mx, at column pos; the others are drawn from (-rel, rel) * mx."""
    r = (_rng(K, pos, *key).uniform(-rel, rel, K) * float(mx)).astype(F32)
    r[pos] = F32(sign) * F32(mx)
    return r


def second_trip_column(K):
    """A column only the SECOND trip of the maximum loop (stride 256) reaches; rows shorter than that: the last column."""
    return 256 + (min(K, 512) - 257) // 2 if K > 256 else K - 1


def edge_rows(K):
    """-> (names, fp32 [n, K]): the rows of the issue, one content per row.  Neighbouring rows differ in their scale's exponent, so a
    scale taken from the row before or behind shows.  No infinity here (inf_rows)."""
    names, rows = [], []

    def add(name, r):
        names.append(name)
        rows.append(np.asarray(r, F32))

    for i, mx in enumerate(scale_edge_maxima()):
        add("max_%s" % np.array([mx], F32).view(np.uint32)[0], _row(K, mx, (5 * i + 1) % K, (1, i), sign=-1.0 if i % 2 else 1.0))
    add("zeros", np.zeros(K, F32))
    tiny = (_rng(K, 2).uniform(-1, 1, K) * 9e-31).astype(F32)  # all below 1e-30: the clamp decides the scale
    den = np.array([1, 0x7FFFFF, 0x400000, 0x80000001, 0x807FFFFF], np.uint32).view(F32)  # fp32 denormals, both signs, both ends
    tiny[(np.arange(len(den)) * 3) % K] = den  # (K = 2: the later ones stay)
    add("below_1e-30_with_denormals", tiny)
    add("all_negative_zero", np.full(K, -0.0, F32))
    r = _row(K, 3.0, K // 2, (3,))
    r[::3] = F32(-0.0)
    r[K // 2] = F32(3.0)
    add("negative_zeros_among_values", r)
    mx = F32(1.37)
    r = np.where(np.arange(K) % 2 == 0, mx * F32(2.0) ** F32(-20) * (1 + _rng(K, 4).uniform(0, 1, K)).astype(F32), -mx * F32(2.0) ** F32(-30)).astype(F32)
    r[K - 1] = mx
    add("entries_2^-20_and_2^-30_of_the_maximum", r)
    # the maximum alone in its column, everything else 2^-3 of it and less: a maximum that is missed moves the exponent
    add("max_at_column_0", _row(K, 2.0 ** 20 * 1.9, 0, (5,), rel=0.1))
    add("max_at_last_column", _row(K, 2.0 ** -20 * 1.1, K - 1, (6,), rel=0.1, sign=-1.0))
    add("max_in_second_trip", _row(K, 2.0 ** 33 * 1.5, second_trip_column(K), (7,), rel=0.1))
    r = _row(K, 0.75, 0, (8,))
    r[1] = NAN
    if K > 2:
        r[K - 2] = -NAN
    add("nan_beside_finite_entries", r)
    return names, np.stack(rows)


def inf_rows(K):
    """fp32 [4, K]: row 1 holds +inf, row 2 -inf among finite entries (some beyond 64, some below 2^-14); rows 0 and 3 are ordinary."""
    w = np.stack([_row(K, 0.3, 1, (11,)), _row(K, 100.0, 0, (12,)), _row(K, 2.0 ** -12, K - 1, (13,)), _row(K, 7.0, 0, (14,))])
    w[1, 1], w[2, 0] = INF, -INF
    return w


def scale_shifts(rows):
    """s in -6 .. 6 per row, every value taken when there are 13 rows or more."""
    return ((np.arange(rows) * 5) % 13 - 6).astype(np.int64)


T_SHAPES = ((2, 1, 1), (2, 3, 3), (32, 1, 32), (34, 2, 33), (64, 27, 8), (6, 32, 40))  # (cout, taps, cin)


def transposed_sels(taps):
    """name -> sel: all taps reversed (the input gradient's filter), a non-monotonic subset (a residue class), a repeated tap, 32 taps."""
    sels = {"reversed": list(range(taps - 1, -1, -1))[:32],
            "subset": [4 % taps, 1 % taps] if taps > 1 else [0],
            "repeated": [taps - 1, 0, taps - 1],
            "nsel32": [(7 * a + 3) % taps for a in range(32)]}
    return sels


def transposed_weight(cout, taps, cin):
    """Values whose bf16 planes differ in every element and whose magnitudes span 2^-8 .. 2^8 (a wrong element cannot pass)."""
    g = _rng(cout, taps, cin, 21)
    return (g.uniform(0.5, 1.0, (cout, taps, cin)) * 2.0 ** g.integers(-8, 9, (cout, taps, cin)) * g.choice([-1.0, 1.0], (cout, taps, cin))).astype(F32)


CLIP_VALUES = np.array([0.0, -0.0, 65504.0, -65504.0, 65519.996, 65520.0, 1e5, -1e5, FLT_MAX, -FLT_MAX, np.inf, -np.inf, np.nan], F32)
CLIP_DENORMALS = np.array([1, 0x7FFFFF, 0x80000001, 0x80400000], np.uint32).view(F32)


def clip_values(shape, key=0):
    """fp32 of `shape`: ordinary pixels with every value of CLIP_VALUES and CLIP_DENORMALS placed round-robin through the array (each
    at least once when the array has room, in every channel over time)."""
    n = int(np.prod(shape))
    x = (_rng(n, key).standard_normal(n) * 2).astype(F32)
    special = np.concatenate([CLIP_VALUES, CLIP_DENORMALS])
    at = np.arange(0, n, 2) if n >= 2 * len(special) else np.arange(n)
    x[at] = special[(np.arange(len(at)) + key) % len(special)]
    return x.reshape(shape)
