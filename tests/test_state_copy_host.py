"""The one-launch state copy (include/avt.h: AvtStateJob, avt_state_job_bytes, avt_state_copy_multi) on the host: the job struct is 32
bytes, and the entry refuses bad arguments before any launch.  No device calls here."""
import ctypes

import pytest
import torch

AVT_ERR_ARG = -1  # include/avt.h


def test_the_job_struct_is_32_bytes_and_the_packer_writes_the_headers_layout(avt):
    import struct

    from avtex import ops, train_ops

    class AvtStateJob(ctypes.Structure):  # include/avt.h
        _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("nbytes", ctypes.c_int64), ("blk0", ctypes.c_int32),
                    ("pad", ctypes.c_int32)]

    assert avt._lib.lib().avt_state_job_bytes() == ops.state_job_bytes() == ctypes.sizeof(AvtStateJob) == 32
    assert struct.calcsize(train_ops._STATE_JOB) == 32


_P = [0x10000 * (i + 1) for i in range(3)]  # made-up device addresses, never dereferenced


# (with made-up addresses a check that went missing would be a real launch: never where a device is visible)
@pytest.mark.skipif(torch.cuda.is_available(), reason="made-up device addresses: only on a box without a GPU")
def test_bad_arguments_are_rejected_before_any_launch(avt):
    lib, checked = avt._lib.lib(), avt._lib.checked
    cases = [
        ((None, _P[1], 4, 0), "NULL pointer"),
        ((_P[0], None, 4, 0), "NULL pointer"),
        ((_P[0], _P[1], 0, 0), "no blocks"),
        ((_P[0], _P[1], -3, 0), "no blocks"),
        ((_P[0] + 4, _P[1], 4, 0), "the job table must be 8-byte aligned"),
        ((_P[0], _P[1] + 2, 4, 0), "the block map 4-byte aligned"),
    ]
    for args, words in cases:
        assert lib.avt_state_copy_multi(*args) == AVT_ERR_ARG, (args, words)
        assert words in lib.avt_last_error().decode(), (args, words, lib.avt_last_error())
        with pytest.raises(avt._lib.AvtError) as e:
            checked.avt_state_copy_multi(*args)
        assert words in str(e.value) and "avt_state_copy_multi" in str(e.value)
