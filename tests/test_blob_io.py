"""tests/blob_io.hpp (the reader, the writer and the main wrapper every stand-alone test program shares) through the tiny program
tests/blob_io_prog.cpp, plain and under the sanitizers, and tests/host_prog.py's own build cache and layout probe."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import host_prog

TYPES = (np.uint8, np.int32, np.int64, np.float32, np.float64)


def blob(sizes, seed=1):
    rng = np.random.default_rng(seed)
    return b"".join(np.array([n], np.int64).tobytes() + rng.integers(0, 256, n * np.dtype(t).itemsize, np.uint8).tobytes()       # (any bit pattern)
                    for n, t in zip(sizes, TYPES))


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def prog(request, tmp_path_factory):
    out_dir = tmp_path_factory.mktemp("blob_io_prog")
    if request.param == "sanitized" and not host_prog.sanitizer_runtime_present(out_dir):
        pytest.skip("the sanitizer runtime (libasan / libubsan) is not installed: a trivial main does not link with -fsanitize")
    return host_prog.build("blob_io_prog", out_dir, sanitize=request.param == "sanitized")


def fails(prog, tmp_path, data, out=None):
    fin = tmp_path / "copy.in"
    fin.write_bytes(data)
    return subprocess.run([prog, "copy", str(fin), str(out or tmp_path / "copy.out")], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("sizes", [(5, 3, 2, 7, 4), (0, 0, 0, 0, 0), (1, 0, 70000, 0, 1)])
def test_round_trip_gives_the_bytes_back(prog, tmp_path, sizes):
    """Arrays of every type, a zero-length array of every type, and an input longer than the reader's 64 KiB chunk."""
    data = blob(sizes)
    assert host_prog.run(prog, tmp_path, "copy", data, timeout=60) == data


def test_input_truncated_by_one_byte_is_reported(prog, tmp_path):
    r = fails(prog, tmp_path, blob((5, 3, 2, 7, 4))[:-1])
    assert r.returncode == 1 and "blob_io_prog: input too short" in r.stderr, (r.returncode, r.stderr[-2000:])


def test_a_hostile_count_is_reported_not_allocated(prog, tmp_path):
    """2^62 elements of 8 bytes: n * sizeof(T) wraps to 0, so a check of at + n * sizeof(T) against the size would pass."""
    head = blob((5, 3, 0, 0, 0))[:8 + 5 + 8 + 12]
    r = fails(prog, tmp_path, head + np.array([2 ** 62], np.int64).tobytes() + bytes(64))
    assert r.returncode == 1 and "blob_io_prog: input too short" in r.stderr, (r.returncode, r.stderr[-2000:])


def test_unwritable_output_path_is_reported(prog, tmp_path):
    r = fails(prog, tmp_path, blob((5, 3, 2, 7, 4)), out=tmp_path / "no_such_directory" / "copy.out")
    assert r.returncode == 1 and "cannot open" in r.stderr, (r.returncode, r.stderr[-2000:])


def test_wrong_argument_count_prints_the_usage(prog):
    for args in ([], ["copy", "only_one"], ["copy", "a", "b", "c"]):
        r = subprocess.run([prog, *args], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "usage: blob_io_prog copy IN OUT" in r.stderr, (args, r.returncode, r.stderr[-2000:])


def test_build_with_the_same_key_compiles_once(tmp_path):
    a = host_prog.build("blob_io_prog", tmp_path, defines=("BLOB_IO_CACHE_TEST",))
    stamp = os.stat(a).st_mtime_ns
    b = host_prog.build("blob_io_prog", tmp_path / "elsewhere", defines=("BLOB_IO_CACHE_TEST",))        # (never created: nothing is compiled)
    assert a == b and os.stat(b).st_mtime_ns == stamp
    assert host_prog.build("blob_io_prog", tmp_path, defines=("BLOB_IO_CACHE_TEST", "OTHER")) != a       # another key, another executable


def test_c_layout_passes_on_the_table_and_fails_on_a_wrong_class(tmp_path):
    from sivo_amd import covisibility
    host_prog.c_layout(tmp_path, "SivoObsTable", covisibility._Table)

    class Wrong(C.Structure):                               # the first field twice its size: every later offset moves
        _fields_ = [(f[0], C.c_int64 if i == 0 else f[1]) for i, f in enumerate(covisibility._Table._fields_)]
    with pytest.raises(AssertionError):
        host_prog.c_layout(tmp_path, "SivoObsTable", Wrong)
