"""Argument checks of the batched BSS Eval path (sk_bss_*, sepkern/bsseval_gpu.py, the --gpu flags): everything
here is rejected before a GPU is touched.  CPU only."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from conftest import PKG


def test_sk_bss_rejects_out_of_range_shapes():
    from sepkern import _lib
    lib = _lib.load()
    offs, lens = (C.c_int64 * 2)(0, 200), (C.c_int32 * 2)(100, 100)
    assert lib.sk_bss_eval(None, None, offs, lens, 2, 5, 512, None, None, None, None) == -1
    assert b"S = 5" in lib.sk_last_error()
    assert lib.sk_bss_xcorr(None, None, offs, lens, 2, 2, 513, None, None, None) == -1
    assert b"taps = 513" in lib.sk_last_error()
    assert lib.sk_bss_eval(None, None, offs, lens, 0, 2, 512, None, None, None, None) == -1
    assert b"U = 0" in lib.sk_last_error()
    bad = (C.c_int32 * 2)(100, 0)
    assert lib.sk_bss_eval(None, None, offs, bad, 2, 2, 512, None, None, None, None) == -1
    assert b"length 0" in lib.sk_last_error()
    assert lib.sk_bss_workspace_bytes(1, 5, 512) == 0 and lib.sk_bss_workspace_bytes(1, 2, 513) == 0
    assert lib.sk_bss_workspace_bytes(3, 2, 512) > 3 * 1024 * 1024 * 8      # three 1024-square Gram matrices at least


def test_batch_raises_the_host_functions_value_errors():
    from sepkern.bsseval_gpu import bss_eval_sources_batch
    x = np.ones((2, 100))
    ok = [np.random.default_rng(0).standard_normal((2, 100))]
    with pytest.raises(ValueError, match="all-zero reference"):
        bss_eval_sources_batch(ok + [np.stack([x[0], np.zeros(100)])], ok + [x])
    with pytest.raises(ValueError, match="all-zero estimated"):
        bss_eval_sources_batch(ok + [x], ok + [np.stack([x[0], np.zeros(100)])])
    with pytest.raises(ValueError, match="same shape"):
        bss_eval_sources_batch(ok + [x], ok + [x[:, :50]])


def test_ops_refuse_cpu_tensors():
    from sepkern import _lib, ops
    t = torch.zeros(200, dtype=torch.float64)
    with pytest.raises(_lib.SepkernError):
        ops.bss_eval(t, t, [0], [100], 2, 512)
    with pytest.raises(_lib.SepkernError):
        ops.bss_xcorr(t, t, [0], [100], 2, 512)


def test_gpu_flags_parse():
    sys.path.insert(0, os.path.join(PKG, "steps"))
    import evaluate_oracle
    import evaluate_sources
    a = evaluate_sources.get_args(["data/test", "exp/x", "--gpu", "--batch", "8"])
    assert a.gpu and a.batch == 8
    assert not evaluate_sources.get_args(["data/test", "exp/x"]).gpu
    a = evaluate_oracle.get_args(["data/test", "--gpu"])
    assert a.gpu and not a.hard_mask
    assert not evaluate_oracle.get_args(["data/test"]).gpu
