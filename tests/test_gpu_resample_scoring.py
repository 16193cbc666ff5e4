"""The two scoring steps on a tree written at 16 kHz: steps/evaluate_oracle.py and steps/evaluate_sources.py resample the
mixture and the references to --sample-rate on the GPU (sk_resample) and score against the resampled signals.  Each is held
against the same computation on the host with sepkern/resample.py's fp64 reference."""
import os
import sys

import numpy as np
import pytest
import scipy.io.wavfile

from conftest import PKG
from oracle import stft as OS

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(PKG, "steps"))


@pytest.fixture(scope="module")
def tree16k(tmp_path_factory):
    """(data dir, ids, {id: [mix, s1, s2] resampled to 8 kHz on the host in fp64}) of a 3-utterance tree written at 16 kHz."""
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    from sepkern import synth
    from sepkern import resample as R
    root = tmp_path_factory.mktemp("score16k")
    wavroot, data = str(root / "wav16k"), str(root / "data")
    ids = synth.write_wav_tree(wavroot, 3, num_spk=2, min_s=1.0, max_s=1.6, rate=16000, seed=7)
    synth.write_data_dir(data, wavroot, ids)
    with open(os.path.join(data, "utt2num_spk"), "w") as f:
        f.write("".join("%s 2\n" % i for i in ids))
    host = {}
    for i in ids:
        host[i] = []
        for d in ("mix", "s1", "s2"):
            fs, x = scipy.io.wavfile.read(os.path.join(wavroot, d, i + ".wav"))
            assert fs == 16000
            host[i].append(R.resample_host(x.astype(np.float64) / 32768.0, 16000, 8000))
    return data, ids, host, root


def _values(path):
    return {l.split(' ')[0]: [float(v) for v in l.split(' ')[1:]] for l in open(path).read().splitlines()}


def test_evaluate_oracle_on_a_16k_tree(tree16k):
    """source_SDRs of the soft oracle mask == the CPU oracle of the same computation (oracle/stft.py, sepkern.bsseval) on the
    host-resampled signals, within the 0.02 dB tests/test_gpu_pipeline.py allows the fp32 kernels against that oracle."""
    import evaluate_oracle
    from sepkern.bsseval import bss_eval_sources
    data, ids, host, _ = tree16k
    evaluate_oracle.main([data])
    got = _values(os.path.join(data, "oracle_soft_mask_eval", "source_SDRs.txt"))
    assert list(got) == ids
    for i in ids:
        mix, srcs = host[i][0], host[i][1:]
        mix_spec = OS.stft(mix)
        mags = [np.abs(OS.stft(p)) for p in srcs]
        ests = np.stack([OS.istft(mix_spec * (m / np.maximum(np.abs(mix_spec), 1e-20))) for m in mags])
        refs = np.stack([p[:ests.shape[1]] for p in srcs])
        sdr, _, _, _ = bss_eval_sources(refs, ests.astype(np.float64), compute_permutation=False)
        np.testing.assert_allclose(got[i], sdr, atol=0.02)


def test_evaluate_sources_on_a_16k_tree(tree16k):
    """Estimates at 8 kHz scored against references on disk at 16 kHz == the same scores taken on the host against the fp64
    resampled references.  The device-resampled references differ from those by fp32 rounding, below 1e-6 of the signal (the
    kernel's bound, tests/test_gpu_resample.py); the estimates' distortion is 0.25 of it, so a score moves by less than
    20 log10(1 + 4e-6) = 4e-5 dB: 1e-3 dB is held."""
    import evaluate_sources
    from sepkern.bsseval import bss_eval_sources
    data, ids, host, root = tree16k
    exp = str(root / "exp")
    ests = {}
    for i in ids:
        s = host[i][1:]
        n = 128 * (len(s[0]) // 128)
        ests[i] = []
        for k in range(2):
            e = np.clip(np.round(32768.0 * (s[k][:n] + 0.25 * s[1 - k][:n])), -32768, 32767).astype(np.int16)
            os.makedirs(os.path.join(exp, "wav", "s%d" % (k + 1)), exist_ok=True)
            scipy.io.wavfile.write(os.path.join(exp, "wav", "s%d" % (k + 1), i + ".wav"), 8000, e)
            ests[i].append(e.astype(np.float64) / 32768.0)
    evaluate_sources.main([data, exp])
    sdrs = _values(os.path.join(exp, "results", "source_SDRs.txt"))
    sis = _values(os.path.join(exp, "results", "source_SISDRs.txt"))
    imps = _values(os.path.join(exp, "results", "source_SISDRis.txt"))
    assert list(sdrs) == ids
    for i in ids:
        e = np.stack(ests[i])
        n = e.shape[1]
        refs = np.stack([p[:n] for p in host[i][1:]])
        sdr, _, _, _ = bss_eval_sources(refs, e)
        np.testing.assert_allclose(sdrs[i], sdr, atol=1e-3)
        si = evaluate_sources.best_si_sdr(e, refs)
        np.testing.assert_allclose(sis[i], si, atol=1e-3)
        from sepkern.sisdr import si_sdr
        np.testing.assert_allclose(imps[i], [v - si_sdr(host[i][0][:n], refs[k]) for k, v in enumerate(si)], atol=1e-3)
