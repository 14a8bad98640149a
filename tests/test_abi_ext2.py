"""The second extension header include/avt_ext2.h (the one-launch state copy) next to include/avt.h and include/avt_ext.h: every entry it
declares is parsed by the same parser, bound and exported; no name lives in two headers; the two pinned tables are untouched; the job
struct is 32 bytes; and the entry refuses bad arguments on the host, before any launch.  No device calls here."""
import ctypes
import re

import pytest
import torch

AVT_ERR_ARG = -1  # include/avt.h


def _declared(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(avt_[a-z0-9_]+)\s*\(", src)))


def test_every_entry_of_the_second_extension_is_parsed_bound_and_exported(avt):
    lib = avt._lib
    names = _declared(lib.EXT2_HEADER_PATH)
    assert sorted(lib.EXT2_SIGNATURES) == names == ["avt_ext2_version", "avt_state_copy_multi", "avt_state_job_bytes"]
    handle = ctypes.CDLL(lib.LIB_PATH)
    for n in names:
        assert hasattr(handle, n), "libavt_hip.so does not export %s" % n
    with open(lib.EXT2_HEADER_PATH) as f:
        text = f.read()
    table = lib.parse_header(text)
    i, vp = ctypes.c_int, ctypes.c_void_p
    assert table["avt_ext2_version"] == (i, []) and table["avt_state_job_bytes"] == (i, [])
    assert table["avt_state_copy_multi"] == (i, [vp, vp, i, vp])
    fn = lib.lib().avt_state_copy_multi  # lib() and `checked` serve the third table, with the header's types
    assert (fn.restype, list(fn.argtypes)) == table["avt_state_copy_multi"]
    assert list(lib.checked.avt_state_copy_multi.argtypes) == table["avt_state_copy_multi"][1]
    assert lib.lib().avt_ext2_version() == lib.EXT2_VERSION == 1
    assert int(re.search(r"#define\s+AVT_EXT2_VERSION\s+(\d+)", text).group(1)) == lib.EXT2_VERSION


def test_no_name_is_shared_and_the_two_pinned_tables_stand(avt):
    lib = avt._lib
    base, ext, ext2 = _declared(lib.HEADER_PATH), _declared(lib.EXT_HEADER_PATH), _declared(lib.EXT2_HEADER_PATH)
    assert not set(ext2) & (set(base) | set(ext)) and not set(base) & set(ext)
    assert not set(lib.EXT2_SIGNATURES) & (set(lib.SIGNATURES) | set(lib.EXT_SIGNATURES) | {"avt_last_error"})
    assert sorted(list(lib.SIGNATURES) + ["avt_last_error"]) == base and len(base) == 122  # SIGNATURES: avt.h alone
    assert sorted(lib.EXT_SIGNATURES) == ext and len(ext) == 7  # EXT_SIGNATURES: avt_ext.h alone
    assert lib.lib().avt_abi_version() == lib.ABI_VERSION == 8 and lib.lib().avt_ext_version() == lib.EXT_VERSION == 1


def test_a_name_declared_in_two_headers_is_an_error(avt, tmp_path, monkeypatch):
    """_lib refuses, at import, a second extension header that declares again what another header declares."""
    import importlib.util
    import shutil

    lib = avt._lib
    pkg = tmp_path / "pkg"
    (tmp_path / "include").mkdir()
    pkg.mkdir()
    shutil.copy(lib.HEADER_PATH, tmp_path / "include" / "avt.h")
    shutil.copy(lib.EXT_HEADER_PATH, tmp_path / "include" / "avt_ext.h")
    with open(lib.EXT2_HEADER_PATH) as f:
        text = f.read()
    (tmp_path / "include" / "avt_ext2.h").write_text(text.replace("int avt_state_job_bytes(void);",
                                                                  "int avt_state_job_bytes(void);\nint avt_sgd_job_bytes(void);"))
    shutil.copy(lib.__file__, pkg / "_lib_copy.py")
    spec = importlib.util.spec_from_file_location("_lib_copy", pkg / "_lib_copy.py")
    mod = importlib.util.module_from_spec(spec)
    with pytest.raises(Exception, match="avt_sgd_job_bytes") as e:
        spec.loader.exec_module(mod)
    assert type(e.value).__name__ == "AvtError" and "avt_ext2.h declares again" in str(e.value)


def test_the_job_struct_is_32_bytes_and_the_packer_writes_the_headers_layout(avt):
    import struct

    from avtex import ops, train_ops

    class AvtStateJob(ctypes.Structure):  # include/avt_ext2.h
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
