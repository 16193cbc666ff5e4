"""The engine's switch table (sepkern.engine._switches): defaults per precision and hidden size, bench.py's fp32_mfma pair,
the errors for malformed values, and the attributes drivers and tests assign on a built engine.  No GPU: an Engine on the CPU
device constructs without the library.  The expected values were read off the engine as it stood before the table existed
(commit ac82019)."""
import pytest
import torch

from sepkern._lib import SepkernError
from sepkern.engine import Engine

SWITCHES = ("SEPKERN_LSTM_MODE", "SEPKERN_LSTM_FWD", "SEPKERN_LSTM_BWD", "SEPKERN_OVERLAP", "SEPKERN_BN_FOLD", "SEPKERN_GEMM_VARIANTS",
            "SEPKERN_WGRAD_PLANES", "SEPKERN_BWD_EXCLUSIVE", "SEPKERN_SYNC_BN")


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


def engine(precision="fp32", hidden=896):
    return Engine(257, 514, hidden, 1, torch.device("cpu"), precision=precision)


@pytest.mark.parametrize("precision, hidden, fwd_bits, bwd_bits, split3_fwd, tagged_fwd, wgrad_planes, bn_fold, nt", [
    ("fp32", 896, 0x10140000, 0x0f840000, True, False, True, True, False),
    ("fp32", 1024, 0x24140000, 0x0f840000, False, True, True, True, False),
    ("bf16", 896, 0x40540000, 0x4f840000, False, False, False, False, True),
    ("fp32", 300, 0x10140000, 0x0f840000, True, False, False, True, False),
])
def test_defaults(precision, hidden, fwd_bits, bwd_bits, split3_fwd, tagged_fwd, wgrad_planes, bn_fold, nt):
    e = engine(precision, hidden)
    assert (e.fwd_bits, e.bwd_bits) == (fwd_bits, bwd_bits), (hex(e.fwd_bits), hex(e.bwd_bits))
    assert (e.split3_fwd, e.tagged_fwd, e.wgrad_planes, e.bn_fold, e.nt) == (split3_fwd, tagged_fwd, wgrad_planes, bn_fold, nt)
    assert (e.var_main, e.var_side) == (0, 2)
    assert e.overlap is True and e.bwd_exclusive == "auto" and e.lstm_mode == 0 and e.sync_bn is False


def test_the_fp32_mfma_pair_of_bench_py(monkeypatch):
    monkeypatch.setenv("SEPKERN_GEMM_VARIANTS", "8,1")
    monkeypatch.setenv("SEPKERN_LSTM_FWD", "0,1,1,0,0,0,0,0")
    e = engine()
    assert e.fwd_bits == 0x00140000 and not e.split3_fwd and not e.tagged_fwd
    assert (e.var_main, e.var_side) == (8, 1)


@pytest.mark.parametrize("name, attr, default", [("SEPKERN_OVERLAP", "overlap", True), ("SEPKERN_BN_FOLD", "bn_fold", True),
                                                 ("SEPKERN_WGRAD_PLANES", "wgrad_planes", True), ("SEPKERN_SYNC_BN", "sync_bn", False)])
def test_one_truth_rule_for_every_on_off_switch(monkeypatch, name, attr, default):
    """"0" = off, any other value = on, unset = the switch's default."""
    assert getattr(engine(), attr) is default
    for value, want in (("0", False), ("1", True), ("true", True)):
        monkeypatch.setenv(name, value)
        assert getattr(engine(), attr) is want, (name, value)


@pytest.mark.parametrize("name, value", [
    ("SEPKERN_GEMM_VARIANTS", "0"), ("SEPKERN_GEMM_VARIANTS", "0,x"), ("SEPKERN_GEMM_VARIANTS", ""),
    ("SEPKERN_GEMM_VARIANTS", "0,2,2"), ("SEPKERN_GEMM_VARIANTS", "0,2,2,2"),        # the retired third / fourth field
    ("SEPKERN_BWD_EXCLUSIVE", "2"), ("SEPKERN_BWD_EXCLUSIVE", "on"),
    ("SEPKERN_LSTM_MODE", "fast"), ("SEPKERN_LSTM_MODE", "1.5"), ("SEPKERN_LSTM_MODE", "0,2"),
    ("SEPKERN_LSTM_FWD", "0,1,a"), ("SEPKERN_LSTM_BWD", "auto"),
])
def test_a_malformed_value_is_an_error_that_names_its_variable(monkeypatch, name, value):
    monkeypatch.setenv(name, value)
    with pytest.raises(SepkernError) as err:
        engine()
    assert name in str(err.value) and repr(value) in str(err.value)


@pytest.mark.parametrize("value, bits", [("auto", "auto"), ("0", "0"), ("1", "1")])
def test_bwd_exclusive_accepts_its_three_values(monkeypatch, value, bits):
    monkeypatch.setenv("SEPKERN_BWD_EXCLUSIVE", value)
    assert engine().bwd_exclusive == bits


def test_lstm_mode_and_the_nine_field_strings_are_read(monkeypatch):
    monkeypatch.setenv("SEPKERN_LSTM_MODE", "2")
    monkeypatch.setenv("SEPKERN_LSTM_BWD", "0,1,0,0,0,31,0,0,1")
    e = engine()
    assert e.lstm_mode == 2 and e.bwd_bits == 0x4f840000


def test_attributes_stay_assignable_on_a_built_engine():
    """bench.py, steps/train_qsub.py and the GPU tests write these between passes; every pass reads them anew."""
    e = engine()
    e.lstm_mode, e.overlap, e.var_main, e.var_side = 2, False, 8, 1
    assert (e.lstm_mode, e.overlap, e.var_main, e.var_side) == (2, False, 8, 1)
    assert e._side(None) is None                    # co-scheduling is decided per pass from the live attributes
    assert not e._planes()                          # ... and so is the arrangement of the weight gradients
    e.var_main, e.var_side = 0, 2
    assert e._planes()
