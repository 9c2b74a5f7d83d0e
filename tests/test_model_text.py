"""CPU: psf_model_write_text, the text format of KVMap::WriteToFile
(src/parameter/kv_map.h:99-117): one `key \\t w \\n` line per pair with
w != 0, the key in decimal and the weight as `std::ostream << float` prints it
(default precision 6, i.e. %g of the promoted value).  No kernel is launched.
"""
import ctypes as C
import os

import numpy as np
import pytest


def _write(path, keys, w, sorted_):
    from parameter_server_amd import lib
    keys = np.ascontiguousarray(keys, np.uint64)
    w = np.ascontiguousarray(w, np.float32)
    assert keys.size == w.size
    return lib().psf_model_write_text(str(path).encode(), keys.ctypes.data_as(C.c_void_p),
                                      w.ctypes.data_as(C.c_void_p), keys.size, sorted_)


def _expected(keys, w):
    return "".join("%d\t%g\n" % (k, float(x)) for k, x in zip(keys.tolist(), w) if x != 0)


@pytest.fixture(scope="module")
def pairs():
    rng = np.random.default_rng(7)
    special_w = np.array([0.0, -0.0, 1e-30, -3.5, 123456789.0, 1e-45, -2e-39, 0.1, 1e10, 100000.0, 1e6,
                          -1.5e-5, 0.0001], np.float32)  # 1e-45 / -2e-39: subnormals
    assert 0 < abs(special_w[5]) < np.finfo(np.float32).tiny
    n = 1000
    keys = np.unique(rng.integers(1, 1 << 63, 2 * n, dtype=np.uint64))[:n - 2]
    keys = np.concatenate([keys, np.array([0, 2**64 - 2], np.uint64)])
    keys = keys[rng.permutation(keys.size)]  # input order is not key order
    w = (rng.standard_normal(keys.size) * np.exp(rng.uniform(-30, 30, keys.size))).astype(np.float32)
    w[rng.choice(keys.size, 100, replace=False)] = 0.0
    w[:special_w.size] = special_w
    assert np.isfinite(w).all() and 0 in keys and np.uint64(2**64 - 2) in keys
    return keys, w


@pytest.mark.parametrize("sorted_", [0, 1])
def test_format_and_order(tmp_path, pairs, sorted_):
    keys, w = pairs
    path = tmp_path / "model.txt"
    assert _write(path, keys, w, sorted_) == 0
    if sorted_:
        o = np.argsort(keys, kind="stable")
        keys, w = keys[o], w[o]
    want = _expected(keys, w)
    assert want.count("\n") == int((w != 0).sum()) < keys.size  # zeros and -0.0 are skipped
    assert open(path).read() == want


def test_zero_pairs_and_all_zero_weights(tmp_path):
    from parameter_server_amd import lib
    path = tmp_path / "empty.txt"
    assert lib().psf_model_write_text(str(path).encode(), None, None, 0, 1) == 0
    assert os.path.getsize(path) == 0
    assert _write(path, [1, 2, 3], [0.0, -0.0, 0.0], 0) == 0
    assert os.path.getsize(path) == 0


def test_creates_the_parent_directory(tmp_path):
    path = tmp_path / "not" / "yet" / "there" / "model_S0"
    assert _write(path, [5, 3], [1.5, -2.0], 1) == 0
    assert open(path).read() == "3\t-2\n5\t1.5\n"


def test_unwritable_path_is_an_error(tmp_path):
    from parameter_server_amd import lib
    from parameter_server_amd._lib import PSF_ERR_ARG
    blocker = tmp_path / "file"
    blocker.write_text("x")
    # the parent is a regular file: neither the directory nor the file can be made
    assert _write(blocker / "sub" / "model.txt", [1], [1.0], 0) == PSF_ERR_ARG
    assert lib().psf_last_error()
    # the path is a directory
    assert _write(tmp_path, [1], [1.0], 0) == PSF_ERR_ARG
    assert lib().psf_last_error()
    assert lib().psf_model_write_text(None, None, None, 0, 0) == PSF_ERR_ARG
