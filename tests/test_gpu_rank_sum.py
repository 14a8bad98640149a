"""csrc/rank_sum.hip through ops.rank_sum on the MI355X: out[i] = parts[0][i] + parts[1][i] + ... + parts[world - 1][i] as ONE fp32 chain
per element in ascending row order, against the same chain in NumPy float32, bit for bit.  Row counts on both sides of the kernel's
four-deep load group and of its remainder loop, lengths that are a tail alone, full lanes with and without a tail, one block and several,
rows that are longer than n; values with exponents 40 binades apart, so that the ORDER of the adds shows in the bits (the test proves on
the host that the descending chain differs); nothing outside [out, out + n) written; NaN, infinities and -0.0; every refused argument.

NaN: IEEE 754 leaves the sign and the payload of a NaN RESULT to the implementation (inf - inf is 0xffc00000 on x86 and 0x7fc00000 on
gfx950), so where the host chain gives a NaN the device must give a NaN, and every other element is compared bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

WORLDS = [1, 2, 3, 4, 5, 8, 9]
LENGTHS = [1, 3, 4, 5, 1023, 1024, 3 * 4096 + 7]
FILL = 0x7FA5A5A5  # the bit pattern out is pre-filled with (a NaN: a read of it would show, too)


def _ceil4(n):
    return (n + 3) // 4 * 4


def _chain(parts, n, order):
    """The fp32 chain over the rows in `order`, every add rounded to float32 on its own."""
    with np.errstate(invalid="ignore", over="ignore"):
        s = parts[order[0], :n].copy()
        for r in order[1:]:
            s = (s + parts[r, :n]).astype(np.float32)
    return s


def _inputs(world, n, ld):
    """parts [world, ld] float32 = randn * 2^randint(-20, 20) per element, NaN past n; for world >= 3 a draw whose descending chain differs
    from the ascending one (the first such seed: a single element need not tell the orders apart) -> (parts, ascending chain)."""
    for seed in range(1000):
        g = np.random.default_rng([world, n, ld, seed])
        parts = (g.standard_normal((world, ld)) * np.exp2(g.integers(-20, 21, (world, ld)))).astype(np.float32)
        parts[:, n:] = np.nan
        want = _chain(parts, n, list(range(world)))
        if world < 3 or not np.array_equal(_chain(parts, n, list(range(world))[::-1]).view(np.int32), want.view(np.int32)):
            return parts, want
    raise AssertionError("no draw in 1000 tells the orders apart (world %d, n %d)" % (world, n))


def _run(avt, dev, parts, n):
    """ops.rank_sum into an out of parts' row length, pre-filled -> out as host int32 bits; the elements past n must keep the fill."""
    ld = parts.shape[1]
    out = torch.full((max(ld, 4),), FILL, dtype=torch.int32, device=dev).view(torch.float32)
    avt.ops.rank_sum(torch.from_numpy(parts).to(dev), out, n)
    torch.cuda.synchronize()
    bits = out.view(torch.int32).cpu().numpy()
    assert (bits[n:] == FILL).all(), "written past n = %d: %s" % (n, np.nonzero(bits[n:] != FILL)[0][:8] + n)
    return bits[:n]


def _assert_bits(got, want):
    nan = np.isnan(want)
    assert np.isnan(got.view(np.float32)[nan]).all()
    bad = np.nonzero((got != want.view(np.int32)) & ~nan)[0]
    assert bad.size == 0, "%d elements differ, first at %s: got %s want %s" % (bad.size, bad[:4], got[bad[:4]], want.view(np.int32)[bad[:4]])


@pytest.mark.parametrize("world", WORLDS)
def test_rows_are_added_in_ascending_order_bit_for_bit(avt, dev, world):
    from avtex import train_ops  # noqa: F401  (the library is loaded the way the package loads it)

    for n in LENGTHS:
        for ld in (_ceil4(n), _ceil4(n) + 8):
            parts, want = _inputs(world, n, ld)
            assert not np.isnan(want).any()
            got = _run(avt, dev, parts, n)
            assert np.array_equal(got, want.view(np.int32)), (world, n, ld, np.nonzero(got != want.view(np.int32))[0][:8])


def test_n_defaults_to_the_length_of_out(avt, dev):
    parts, want = _inputs(3, 1024, 1024)
    out = torch.empty(1024, dtype=torch.float32, device=dev)
    avt.ops.rank_sum(torch.from_numpy(parts).to(dev), out)
    assert np.array_equal(out.cpu().numpy().view(np.int32), want.view(np.int32))


@pytest.mark.parametrize("what", ["nan", "inf", "negative-zero"])
def test_special_values(avt, dev, what):
    """n = 23: five full lanes and a tail of three, specials in both; 5 rows: a full load group and the remainder loop."""
    world, n, ld = 5, 23, 24
    parts, _ = _inputs(world, n, ld)
    if what == "nan":
        parts[0, 1] = parts[2, 6] = parts[4, 21] = np.nan  # in the first row, inside the group, in the remainder row; lane and tail
    elif what == "inf":
        parts[1, 2] = parts[4, 20] = np.inf      # inf + finite = inf
        parts[3, 5] = parts[0, 22] = -np.inf
        parts[0, 9], parts[3, 9] = np.inf, -np.inf   # inf - inf: a NaN
        parts[2, 21], parts[4, 21] = -np.inf, np.inf
    else:
        parts[:, 3] = parts[:, 22] = -0.0        # -0 + -0 = -0: the sign survives the whole chain
        parts[:, 7] = -0.0
        parts[2, 7] = 0.0                        # -0 + +0 = +0
    want = _chain(parts, n, list(range(world)))
    if what == "inf":
        assert np.isnan(want[9]) and np.isnan(want[21]) and want[2] == np.inf and want[22] == -np.inf
    if what == "nan":
        assert np.isnan(want[[1, 6, 21]]).all() and np.isnan(want).sum() == 3
    if what == "negative-zero":
        assert want.view(np.int32)[3] == want.view(np.int32)[22] == np.int32(-2 ** 31) and want.view(np.int32)[7] == 0
    _assert_bits(_run(avt, dev, parts, n), want)
    # world 1 is a copy: every bit of the row, the payload of a NaN and the sign of a zero included
    row = parts[2:3].copy()
    row[0, 4] = np.array([0x7FC12345], np.int32).view(np.float32)[0]
    assert np.array_equal(_run(avt, dev, row, n), row[0, :n].view(np.int32))


def test_bad_arguments_raise_before_any_launch(avt, dev):
    """Every refusal of the header, through the checked entry on real device buffers: out keeps its fill."""
    K, AvtError = avt._lib.checked, avt._lib.AvtError
    parts = torch.zeros((3, 16), dtype=torch.float32, device=dev)
    out = torch.full((16,), FILL, dtype=torch.int32, device=dev).view(torch.float32)
    p, o, st = parts.data_ptr(), out.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    big = (1 << 31) * 1024  # 2^31 blocks of 256 threads x 4 floats
    cases = [
        ((None, 3, 16, 16, o), "NULL pointer"),
        ((p, 3, 16, 16, None), "NULL pointer"),
        ((p, 0, 16, 16, o), "world must be >= 1"),
        ((p, -2, 16, 16, o), "world must be >= 1"),
        ((p, 3, -1, 16, o), "n >= 0"),
        ((p, 3, 16, 12, o), "cover n"),
        ((p, 3, 10, 14, o), "multiple of 4"),
        ((p + 4, 3, 8, 8, o), "16-byte aligned"),
        ((p, 3, 8, 16, o + 8), "16-byte aligned"),
        ((p, 3, big, big, o), "2^31 - 1 blocks"),
    ]
    for args, words in cases:
        with pytest.raises(AvtError, match="avt_rank_sum_f32") as e:
            K.avt_rank_sum_f32(*args, st)
        assert words in str(e.value), (args, str(e.value))
    assert avt._lib.lib().avt_rank_sum_f32(p, 3, big - 4, big, o, st) == -1  # (2^31 - 1 full blocks fit; a 2^31st, partly filled, does not)
    K.avt_rank_sum_f32(p, 3, 0, 16, o, st)  # n == 0: AVT_OK, no launch
    K.avt_rank_sum_f32(p, 3, 0, 0, o, st)
    torch.cuda.synchronize()
    assert bool((out.view(torch.int32) == FILL).all())


def test_the_wrapper_rejects_host_tensors_and_overlap(avt, dev):
    AvtError = avt._lib.AvtError
    parts = torch.zeros((2, 8), dtype=torch.float32, device=dev)
    out = torch.zeros(8, dtype=torch.float32, device=dev)
    with pytest.raises(AvtError, match="device"):
        avt.ops.rank_sum(parts.cpu(), out)
    with pytest.raises(AvtError, match="device"):
        avt.ops.rank_sum(parts, out.cpu())
    with pytest.raises(AvtError):
        avt.ops.rank_sum(parts.double(), out)
    with pytest.raises(AvtError, match="world, ld"):
        avt.ops.rank_sum(parts.reshape(-1), out)
    with pytest.raises(AvtError, match="disjoint"):
        avt.ops.rank_sum(parts, parts[1])
    with pytest.raises(AvtError, match="holds 8"):
        avt.ops.rank_sum(parts, out, 9)
