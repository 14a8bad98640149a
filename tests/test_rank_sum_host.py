"""The ordered exchange on the host: avt_rank_sum_f32 (include/avt.h) refuses every bad argument before any launch, n == 0 is AVT_OK
without one, and train_ops.GradExchange takes `ordered`.  No device calls here."""
import pytest
import torch

AVT_OK, AVT_ERR_ARG = 0, -1  # include/avt.h

_P = [0x10000 * (i + 1) for i in range(2)]  # made-up device addresses, never dereferenced


# (with made-up addresses a check that went missing would be a real launch: never where a device is visible)
@pytest.mark.skipif(torch.cuda.is_available(), reason="made-up device addresses: only on a box without a GPU")
def test_bad_arguments_are_rejected_before_any_launch(avt):
    lib, checked = avt._lib.lib(), avt._lib.checked
    big = (1 << 31) * 1024  # 2^31 blocks of 256 threads x 4 floats
    cases = [
        ((None, 3, 16, 16, _P[1], 0), "NULL pointer"),
        ((_P[0], 3, 16, 16, None, 0), "NULL pointer"),
        ((_P[0], 0, 16, 16, _P[1], 0), "world must be >= 1"),
        ((_P[0], 3, -1, 16, _P[1], 0), "n >= 0"),
        ((_P[0], 3, 17, 16, _P[1], 0), "cover n"),
        ((_P[0], 3, 10, 14, _P[1], 0), "multiple of 4"),
        ((_P[0] + 4, 3, 8, 8, _P[1], 0), "16-byte aligned"),
        ((_P[0], 3, 8, 8, _P[1] + 8, 0), "16-byte aligned"),
        ((_P[0], 3, big, big, _P[1], 0), "2^31 - 1 blocks"),
        ((_P[0], 3, big - 4, big, _P[1], 0), "2^31 - 1 blocks"),
        ((None, 3, 0, 16, _P[1], 0), "NULL pointer"),  # (the checks come before the n == 0 return)
    ]
    for args, words in cases:
        assert lib.avt_rank_sum_f32(*args) == AVT_ERR_ARG, (args, words)
        assert words in lib.avt_last_error().decode(), (args, words, lib.avt_last_error())
        with pytest.raises(avt._lib.AvtError) as e:
            checked.avt_rank_sum_f32(*args)
        assert words in str(e.value) and "avt_rank_sum_f32" in str(e.value)
    assert lib.avt_rank_sum_f32(_P[0], 3, 0, 16, _P[1], 0) == AVT_OK  # n == 0: no launch (there is no device here to launch on)
    assert lib.avt_rank_sum_f32(_P[0], 1, 0, 0, _P[1], 0) == AVT_OK


def test_the_entry_keeps_its_signature(avt):
    """The entry's record, in the form of tests/golden/abi_entries.txt's lines (`name restype argtypes...` in ctypes type names): the
    header declares it with exactly that signature, the binding carries it, and the library loaded is built from this header."""
    import ctypes as C

    recorded = "avt_rank_sum_f32 c_int c_void_p c_int c_int64 c_int64 c_void_p c_void_p".split()
    names = {getattr(C, n): n for n in ("c_int", "c_int64", "c_float", "c_double", "c_size_t", "c_void_p", "c_char_p")}
    with open(avt._lib.HEADER_PATH) as f:
        table = avt._lib.parse_header(f.read())
    restype, argtypes = table[recorded[0]]
    assert [names[t] for t in [restype] + list(argtypes)] == recorded[1:]
    assert avt._lib.SIGNATURES[recorded[0]] == argtypes
    fn = getattr(avt._lib.lib(), recorded[0])
    assert (fn.restype, list(fn.argtypes)) == (restype, argtypes)
    assert avt._lib.ABI_VERSION == avt._lib.lib().avt_abi_version()


def test_the_wrapper_rejects_host_tensors(avt):
    with pytest.raises(avt._lib.AvtError, match="device"):
        avt.ops.rank_sum(torch.zeros(2, 8), torch.zeros(8))


def test_grad_exchange_takes_ordered_and_counts_the_sum(avt):
    from avtex import train_ops

    assert train_ops.CALLS["rank_sum"] == 0 or isinstance(train_ops.CALLS["rank_sum"], int)
    p = torch.nn.Parameter(torch.zeros(3))
    for ordered in (None, True, False):
        ex = train_ops.GradExchange([p], 3, ordered=ordered)
        assert ex.ordered is ordered and ex.parts is None and not ex.bound
        with pytest.raises(avt._lib.AvtError, match="before bind"):
            ex.exchange()
