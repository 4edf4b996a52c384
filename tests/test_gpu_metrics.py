"""GPU: the validation metrics (csrc/metrics.hip, avr_amd/metrics.py) against
golden vectors of the reference's own utils/metric.py (tests/golden/metrics,
written by tools/gen_metrics_golden.py) and, for the multi-resolution STFT
term, against the CPU restatement oracle/criterion_oracle.py (auraloss is
absent: that term stays parity-unpinned, as the criterion's is).

Tolerances: Angle, Amplitude, Envelope, T60 and C50 errors within
1e-4 |ref| + 1e-7 of the reference (the bar of test_gpu_criterion.py; the
reference's own fp32-input and fp64-input results differ by <= 5e-7
relative on these inputs); the EDT error within 6 / fs (one nearest-sample
flip); the energy curves within 1e-3 dB where the reference is above -60 dB.
Each test prints its figures before it asserts."""
import json

import numpy as np
import pytest
import torch

import avr_amd
from avr_amd.criterion import Criterion
from avr_amd.metrics import METRIC_KEYS, MetricAccumulator, calculate_metrics, metric_cal, metric_rows
from criterion_cases import RAF_W, RENDER, spectra
from metrics_cases import CASES, WINDOW, irs, load, restate
from oracle import criterion_oracle as co

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
NAMES = ("angle", "amplitude", "envelope", "t60", "edt", "c50")


def _dev(a):
    return torch.from_numpy(a).to(DEV)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_metrics_match_reference_fixture(case):
    name, B, n, fs, seed, noise, delay = case
    z = load(name)
    ori, pred = irs(B, n, seed, noise, delay)
    out = metric_cal(_dev(ori), _dev(pred), fs=fs, window=WINDOW)
    assert len(out) == 9
    assert all(x.is_cuda and x.dim() == 0 for x in out[:7])
    assert out[7].shape == (B, n) and out[8].shape == (B, n)
    got = [float(x) for x in out[:6]]
    ref = z["metrics"]
    for i, key in enumerate(NAMES):
        print(f"{name} {key}: gpu {got[i]!r} ref {ref[i]!r} rel {abs(got[i] - ref[i]) / max(abs(ref[i]), 1e-30):.2e}")
    for which, g, r in (("ori", out[7], z["ori_energy"]), ("pred", out[8], z["pred_energy"])):
        mask = r > -60.0
        err = np.abs(g.cpu().numpy() - r)[mask].max()
        print(f"{name} {which}_energy: max err above -60 dB {err:.2e} dB")
        assert err <= 1e-3, (name, which, err)
    for i, key in enumerate(NAMES):
        if np.isnan(ref[i]):
            assert np.isnan(got[i]), (name, key, got[i])
        elif key == "edt":
            assert abs(got[i] - ref[i]) <= 6.0 / fs, (name, key, got[i], ref[i])
        else:
            assert abs(got[i] - ref[i]) <= 1e-4 * abs(ref[i]) + 1e-7, (name, key, got[i], ref[i])
    # per-row T60 / EDT of both signals
    rows = metric_rows(_dev(ori), _dev(pred), fs=fs, window=WINDOW).cpu().numpy()
    t60 = rows[:, 0:2].T
    edt = rows[:, 2:4].T
    print(f"{name} rows: t60 rel {np.abs(t60 - z['t60_rows']).max() / np.abs(z['t60_rows']).max():.2e} "
          f"edt abs {np.abs(edt - z['edt_rows']).max():.2e}")
    assert np.all(np.abs(t60 - z["t60_rows"]) <= 1e-4 * np.abs(z["t60_rows"]))
    assert np.all(np.abs(edt - z["edt_rows"]) <= 6.0 / fs + 1e-6)


@pytest.mark.parametrize("case", CASES[:4], ids=[c[0] for c in CASES[:4]])
def test_multi_stft_matches_oracle(case):
    name, B, n, fs, seed, noise, delay = case
    ori, pred = irs(B, n, seed, noise, delay)
    x, y = torch.from_numpy(ori).unsqueeze(1), torch.from_numpy(pred).unsqueeze(1)
    ref = sum(float(co.stft_loss(x, y, nfft, hop, win))
              for nfft, hop, win in ((512, 60, 300), (256, 30, 150), (128, 8, 75))) / 3.0
    got = float(metric_cal(_dev(ori), _dev(pred), fs=fs)[6])
    print(f"{name} multi_stft: gpu {got!r} oracle {ref!r} rel {abs(got - ref) / abs(ref):.2e}")
    assert abs(got - ref) <= 1e-4 * abs(ref)


# shapes the fixtures do not reach: the longest legal IR (LDS arrays full, 48
# samples per lane in the scan), a bin count one short of a staging round
# (n/2 + 1 = 1023), odd windows, and a window as long as the IR
EDGE = [(1, 12288, 16000, 32), (2, 2044, 16000, 33), (2, 1022, 24000, 7), (2, 1022, 24000, 1022),
        (2, 258, 4000, 1)]


@pytest.mark.parametrize("B,n,fs,window", EDGE, ids=[f"{c[1]}w{c[3]}" for c in EDGE])
def test_edge_shapes_match_the_float64_restatement(B, n, fs, window):
    """Against metrics_cases.restate (numpy, float64), which
    tests/test_metrics_cpu.py pins to the reference's fixtures within 1e-6
    and which agrees with scipy's convolve1d for odd and even windows; same
    bars as the fixture test."""
    ori, pred = irs(B, n, 11)
    angle, amp, env, oe, pe = restate(ori, pred, fs, window)
    out = metric_cal(_dev(ori), _dev(pred), fs=fs, window=window)
    for key, g, r in (("angle", out[0], angle), ("amplitude", out[1], amp), ("envelope", out[2], env)):
        g = float(g)
        print(f"n={n} w={window} {key}: gpu {g!r} restated {r!r} rel {abs(g - r) / abs(r):.2e}")
    for g, r in ((out[7], oe), (out[8], pe)):
        err = np.abs(g.cpu().numpy() - r)[r > -60.0].max()
        print(f"n={n} energy: max err above -60 dB {err:.2e} dB")
        assert err <= 1e-3
    for g, r in ((out[0], angle), (out[1], amp), (out[2], env)):
        assert abs(float(g) - r) <= 1e-4 * abs(r) + 1e-7
    assert all(bool(torch.isfinite(x)) for x in (out[3], out[4]))


def test_degenerate_row_is_nan_and_neighbours_are_unaffected():
    """A row that is a single impulse at its last sample: its curve is flat,
    the -5 and -25 dB samples coincide (the reference's linregress raises
    there), so its T60 is NaN and its EDT 0; the rows beside it keep the
    values they have without it."""
    B, n, fs = 3, 258, 4000
    ori, pred = irs(B, n, 4)
    clean = metric_rows(_dev(ori), _dev(pred), fs=fs)
    ori2 = ori.copy()
    ori2[1] = 0.0
    ori2[1, n - 1] = 1.0
    rows = metric_rows(_dev(ori2), _dev(pred), fs=fs)
    out = metric_cal(_dev(ori2), _dev(pred), fs=fs)
    torch.cuda.synchronize()
    print("degenerate row:", rows[1].tolist())
    assert torch.isnan(rows[1, 0]) and float(rows[1, 2]) == 0.0
    assert torch.equal(_bits(rows[0]), _bits(clean[0])) and torch.equal(_bits(rows[2]), _bits(clean[2]))
    assert torch.equal(_bits(rows[1, 1::2][:3]), _bits(clean[1, 1::2][:3]))  # pred's T60, EDT, C50
    assert torch.isnan(out[3])  # the batch's T60 error carries the NaN
    assert float(out[7][1].abs().max()) == 0.0  # a flat curve


def test_results_repeat_bitwise_and_rows_do_not_depend_on_the_batch():
    B, n, fs = 4, 1600, 16000
    ori, pred = irs(B, n, 1)
    o, p = _dev(ori), _dev(pred)
    a = metric_cal(o, p, fs=fs)
    b = metric_cal(o, p, fs=fs)
    assert _same(a, b)
    rows = metric_rows(o, p, fs=fs)
    for i in range(B):
        one = metric_rows(o[i], p[i], fs=fs)  # 1-D input: one row
        assert one.shape == (1, 9)
        assert torch.equal(_bits(one[0]), _bits(rows[i])), i
    # the batch means are the rows' means
    means = torch.stack(a[:3]).cpu().double()
    want = rows[:, 6:9].cpu().double().sum(0) / (B * n)
    assert torch.allclose(means, want, rtol=1e-6, atol=0)


def test_metric_cal_is_capturable_in_a_graph():
    """No sync, no device-to-host copy, no allocation outside torch's caching
    allocator after the first call: one call captures into a graph and its
    replay equals the eager result bitwise."""
    B, n, fs = 2, 1022, 24000
    ori, pred = irs(B, n, 0)
    o, p = _dev(ori), _dev(pred)
    eager = metric_cal(o, p, fs=fs)  # warm-up: builds the tables
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = metric_cal(o, p, fs=fs)
    g.replay()
    torch.cuda.synchronize()
    assert _same(eager, captured)


def test_cpu_tensors_and_bad_shapes_raise():
    ori, pred = irs(2, 1022, 0)
    with pytest.raises(RuntimeError, match="HIP tensor"):
        metric_cal(torch.from_numpy(ori), torch.from_numpy(pred))
    with pytest.raises(RuntimeError, match="even"):
        metric_cal(_dev(ori)[:, :1021], _dev(pred)[:, :1021])
    with pytest.raises(RuntimeError, match="256 < n"):
        metric_cal(_dev(ori)[:, :256], _dev(pred)[:, :256])
    with pytest.raises(RuntimeError, match="window"):
        metric_cal(_dev(ori), _dev(pred), window=1024)


def test_calculate_metrics_and_accumulator():
    B, F, fs = 4, 801, 16000
    crit = Criterion(RAF_W, RENDER)
    per_batch = []
    acc = MetricAccumulator()
    for seed in (1, 2, 3):
        pred, ori = spectra(B, F, seed)
        p, o = pred.to(DEV), ori.to(DEV)
        losses, metrics, ori_time, pred_time = calculate_metrics(crit, p, o, fs)
        ref = crit(p, o)
        want = dict(spec_loss=ref[0], fft_loss=ref[1] + ref[2], time_loss=ref[3], energy_loss=ref[4],
                    multi_stft_loss=ref[5], das_reg_loss=ref[6], das_ce_loss=ref[7])
        assert list(losses) == list(want)
        for k in want:
            assert torch.equal(_bits(losses[k]), _bits(want[k])), k
        assert torch.equal(_bits(ori_time), _bits(ref[8])) and torch.equal(_bits(pred_time), _bits(ref[9]))
        m = metric_cal(ref[8], ref[9], fs=fs)
        assert tuple(metrics) == METRIC_KEYS
        for k, v in zip(("Angle", "Amplitude", "Envelope", "T60", "EDT", "C50", "multi_stft"), m[:7]):
            assert torch.equal(_bits(metrics[k]), _bits(v)), k
        acc.add(metrics)
        per_batch.append([float(metrics[k]) for k in METRIC_KEYS])
    avg, std = acc.result()
    per = np.array(per_batch, np.float64)
    assert len(acc) == 3
    for i, k in enumerate(METRIC_KEYS):
        assert abs(avg[k] - per[:, i].mean()) <= 1e-6 * abs(per[:, i].mean()), k
        assert abs(std[k] - np.std(per[:, i])) <= 1e-5 * np.std(per[:, i]) + 1e-9, k
    assert avr_amd.metric_cal is metric_cal and avr_amd.MetricAccumulator is MetricAccumulator


def test_fixture_meta_names_the_case():
    for name, B, n, fs, *_ in CASES:
        meta = json.loads(str(load(name)["meta"]))
        assert (meta["name"], meta["B"], meta["n"], meta["fs"]) == (name, B, n, fs)
