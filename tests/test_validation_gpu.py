"""GPU: the validation epoch on the device (dcsnet/validation.py, csrc/validation.hip) — the accumulator kernel against the host
restatement of its rule, DeviceValidator against fit.validate for both networks, the captured route against the eager one and
across a train step (no stale graph), fit(validation='device') against fit(validation='host'), and extended=True.

LOSS PARITY MARGIN.  The host route evaluates a batch's losses by val_batch_2_metric_loss (the unfused step), the device route by
the step train_batch_2_loss takes (the fused pair route).  At the parent commit 354386c, on this file's batches (five pairs,
batch 2, the crops of epoch 3, seeded weights), the two were evaluated under no_grad in eval mode on an MI355X
(profiles/validation_parity.txt): the largest relative difference |a - b| / max(|a|, |b|) over the batches and the three losses
was 0.0 for C_NETWORK ('dcs' and 'dc': bit-equal batch by batch) and 1.041e-07 for R_NETWORK ('drs'): MEASURED_REL below.  The
margin is 4 x the largest, 4.2e-07, which the tail tests' floor of 2e-6 replaces (fp32 losses: the float32 mean of batch means
fit.validate takes against the device route's fp64 one is itself worth an ulp or two, 3e-8 to 7e-8 seen here).

With bf16 activation storage the same measurement gives 2.022e-04 (MEASURED_REL_BF16): at the parent, the first forward of a
bf16-storage network after set_activation_dtype differs from its later forwards on the same batch by that much in the losses (the
first batch's rows of profiles/validation_parity.txt; the later batches are bit-equal between the routes).  The bf16 test alone
uses 4 x that; the fp32 tests keep MARGIN."""
import json
import math
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.seeded_state import fill_state, fill_state_stream   # noqa: E402

MEASURED_REL = {'dcs': 0.0, 'drs': 1.041e-07, 'dc': 0.0}    # parent 354386c, profiles/validation_parity.txt
MARGIN = max(4 * max(MEASURED_REL.values()), 2e-6)
MEASURED_REL_BF16 = 2.022e-04                               # the same measurement with bf16 activation storage ('dcs-bf16' rows)
MARGIN_BF16 = max(4 * MEASURED_REL_BF16, 2e-6)
SEED, EPOCH, BATCH = 11, 3, 2
LOSS_KEYS = ('val_loss', 'val_noise_loss', 'val_speech_loss')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from dcsnet import _lib
    _lib.load()
    return torch.device('cuda:0')


def _pairs():
    """Six clean / noisy pairs of 0.6 to 1.0 s at 48 kHz as 16-bit PCM, as tests/test_fit_gpu.py::_pairs."""
    rng = np.random.default_rng(4)
    clean, noisy = [], []
    for i, sec in enumerate((0.6, 0.7, 0.8, 0.9, 1.0, 0.75)):
        t = np.arange(int(sec * 48000)) / 48000
        x = 0.3 * np.sin(2 * np.pi * (200 + 90 * i) * t) * (0.6 + 0.4 * np.sin(2 * np.pi * (3 + i) * t))
        y = x + 0.05 * rng.standard_normal(len(t))
        clean.append(np.round(x * 32767).astype(np.int16))
        noisy.append(np.round(np.clip(y, -1, 1) * 32767).astype(np.int16))
    return clean, noisy


@pytest.fixture(scope='module')
def stores(dev):
    """(five pairs: batches of 2, 2 and 1; the first four: the training items of the fit test)"""
    from dcsnet.audio_store import DeviceAudioStore
    from dcsnet.config import config
    clean, noisy = _pairs()
    return DeviceAudioStore(clean[:5], noisy[:5], config, dev), DeviceAudioStore(clean[:4], noisy[:4], config, dev)


@pytest.fixture(scope='module')
def host_stoi():
    """network_functions.stoi -> metrics.stoi for the module: the host side is the project's contract even where pystoi exists."""
    from dcsnet import metrics, network_functions
    saved = network_functions.stoi
    network_functions.stoi = metrics.stoi
    yield
    network_functions.stoi = saved


class _Mode:
    """sys.argv[1] as the model code reads it, set and restored."""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        self.argv = sys.argv
        sys.argv = ['train.py', self.mode, '0']

    def __exit__(self, *exc):
        sys.argv = self.argv


def _cnet(dev):
    from dcsnet.c_network import C_NETWORK
    from dcsnet.config import config, hparams
    return fill_state(C_NETWORK(config, dict(hparams), 0), 7).to(dev).train()


def _rnet(dev):
    from dcsnet.config import config, hparams
    from dcsnet.r_network import R_NETWORK
    return fill_state_stream(R_NETWORK(config, dict(hparams), 0), 7).to(dev).train()


def _close(a, b, margin=MARGIN):
    return abs(a - b) <= margin * max(abs(a), abs(b))


def _check_losses(got, want, keys=LOSS_KEYS, margin=MARGIN):
    for k in keys:
        print(f'{k}: {got[k]!r} vs {want[k]!r}: rel {abs(got[k] - want[k]) / max(abs(got[k]), abs(want[k])):.3e} (margin {margin:.1e})')
    for k in keys:
        assert math.isfinite(got[k]) and _close(got[k], want[k], margin), (k, got[k], want[k])


@pytest.fixture(scope='module')
def dcs(dev, stores, host_stoi):
    """The shared references on the seeded C network, computed once: fit.validate and the eager device route, epoch 3."""
    from dcsnet.fit import validate
    from dcsnet.validation import DeviceValidator
    with _Mode('dcs'):
        net = _cnet(dev)
        host = validate(net, stores[0], BATCH, SEED, EPOCH)
        v = DeviceValidator(net, stores[0], BATCH, seed=SEED, use_graph=False)
        eager = v.run(EPOCH)
        assert net.training and getattr(net, '_dcs_skip_flag', None) is None
    return net, host, eager, dict(v.counts)


# ---- 1. the accumulator alone ------------------------------------------------------------------------------------------------

def _sequence(B, n_loss, n_scores, seed, batches=7):
    """Hand-planted batches as float32 arrays: batch 1 a NaN monitored loss, batch 2 +Inf, batch 3 NaN scores at lanes 0, 63, 64
    and B - 1, batch 4 an all-NaN first score row."""
    rng = np.random.default_rng(seed)
    rows = []
    for b in range(batches):
        losses = rng.uniform(-20, 5, n_loss).astype(np.float32)
        scores = rng.uniform(0, 1, (n_scores, B)).astype(np.float32)
        if b == 1:
            losses[-1] = np.nan
        if b == 2:
            losses[-1] = np.inf
        if b == 3 and n_scores:
            for lane in (0, 63, 64, B - 1):
                if lane < B:
                    scores[:, lane] = np.nan
        if b == 4 and n_scores:
            scores[0, :] = np.nan
        rows.append((losses, scores))
    return rows


def _run_sequence(rows, dev):
    from dcsnet import ops
    state = torch.zeros(ops.VAL_STATE, dtype=torch.float64, device=dev)
    for losses, scores in rows:
        ops.val_accumulate(torch.from_numpy(losses).to(dev), torch.from_numpy(scores).to(dev) if len(scores) else None, state)
    return state.cpu().tolist()


def _check_state(got, rows, B, n_loss, n_scores):
    from dcsnet import ops
    from dcsnet.validation import epoch_means, fold_batches
    ref = fold_batches([(lo.tolist(), sc.tolist()) for lo, sc in rows])
    u = 2.0 ** -53
    kept_rows = [(lo, sc) for lo, sc in rows if not np.isnan(lo[-1])]
    for i in [ops.VAL_KEPT, ops.VAL_SKIPPED] + [ops.VAL_SCORE_NAN + r for r in range(ops.VAL_MAX_SCORES)]:
        assert got[i] == ref[i], (i, got[i], ref[i])                            # counts: exact
    assert (ref[ops.VAL_KEPT], ref[ops.VAL_SKIPPED]) == (len(rows) - 1, 1)
    bounds = {}
    for k in range(n_loss):                                                       # |got - ref| <= 4 n 2^-53 sum|x|
        x = [abs(float(lo[k])) for lo, _ in kept_rows]
        bounds[ops.VAL_LOSS_SUM + k] = 4 * len(x) * u * sum(x)
    for r in range(n_scores):                                                     # n: B addends per batch mean, then the batches
        x = [float(np.nansum(np.abs(sc[r].astype(np.float64)))) / max(int((~np.isnan(sc[r])).sum()), 1) for _, sc in kept_rows]
        bounds[ops.VAL_SCORE_SUM + r] = 4 * (B + len(x)) * u * sum(x)
    for i, bound in bounds.items():
        if math.isfinite(ref[i]):
            assert abs(got[i] - ref[i]) <= bound, (i, got[i], ref[i], bound)
        else:
            assert got[i] == ref[i] or (got[i] != got[i] and ref[i] != ref[i]), (i, got[i], ref[i])
    for i in range(ops.VAL_STATE):                                                # nothing else is touched
        if i not in bounds and i not in (ops.VAL_KEPT, ops.VAL_SKIPPED) and not ops.VAL_SCORE_NAN <= i < ops.VAL_SCORE_NAN + 4:
            assert got[i] == 0.0, i
    gm, rm = epoch_means(got, n_loss, n_scores), epoch_means(ref, n_loss, n_scores)
    kept = ref[ops.VAL_KEPT]
    for g, r_, i in zip(gm[0] + gm[1], rm[0] + rm[1], list(range(n_loss)) + [ops.VAL_SCORE_SUM + r for r in range(n_scores)]):
        if math.isfinite(r_):
            assert abs(g - r_) <= bounds[i] / kept + abs(r_) * 2 * u, (i, g, r_)
        else:
            assert g == r_ or (g != g and r_ != r_)
    assert math.isinf(rm[0][n_loss - 1])                                          # the +Inf batch was kept and propagates


@pytest.mark.parametrize('n_scores', [0, 1, 2])
@pytest.mark.parametrize('n_loss', [1, 3])
@pytest.mark.parametrize('B', [1, 63, 64, 65, 257, 1000])
def test_accumulator_against_the_host_fold(dev, B, n_loss, n_scores):
    first = _sequence(B, n_loss, n_scores, seed=B * 10 + n_loss + n_scores)
    _check_state(_run_sequence(first, dev), first, B, n_loss, n_scores)
    second = _sequence(B, n_loss, n_scores, seed=5000 + B, batches=6)            # a zeroed state does not see the first sequence
    _check_state(_run_sequence(second, dev), second, B, n_loss, n_scores)


def test_accumulator_skips_every_batch_of_nan_losses(dev):
    from dcsnet import ops
    rows = [(np.array([1.0, 2.0, np.nan], np.float32), np.ones((1, 5), np.float32))] * 3
    got = _run_sequence(rows, dev)
    assert got[ops.VAL_SKIPPED] == 3 and sum(abs(v) for v in got) == 3


# ---- 2. device against host, C_NETWORK 'dcs' ----------------------------------------------------------------------------------

def test_device_route_matches_fit_validate(dcs):
    _, host, eager, counts = dcs
    assert list(eager) == list(host) == ['val_loss', 'val_noise_loss', 'val_speech_loss', 'val_pesq', 'val_stoi']
    assert all(isinstance(v, float) for v in eager.values())
    assert math.isnan(eager['val_pesq']) and math.isnan(host['val_pesq'])
    print(f"val_stoi: {eager['val_stoi']!r} vs {host['val_stoi']!r}")
    assert abs(eager['val_stoi'] - host['val_stoi']) <= 1e-4
    _check_losses(eager, host)
    assert counts == {'batches': 3, 'skipped': 0, 'nan_scores': 0}


# ---- 3. captured against eager, and no stale graph ----------------------------------------------------------------------------

def test_captured_route_matches_eager_and_recaptures_after_a_train_step(dev, stores, dcs):
    from dcsnet.dp import TrainStep
    from dcsnet.validation import DeviceValidator
    _, _, eager, _ = dcs
    with _Mode('dcs'):
        net = _cnet(dev)                                                          # the fixture's weights again
        v = DeviceValidator(net, stores[0], BATCH, seed=SEED, use_graph=True)
        first = v.run(EPOCH)
        graph = v._graph
        assert graph is not None
        _check_losses(first, eager)
        assert abs(first['val_stoi'] - eager['val_stoi']) <= 1e-4
        again = v.run(EPOCH)                                                       # nothing changed: the same graph, the same books
        assert v._graph is graph
        assert all(again[k] == first[k] for k in LOSS_KEYS + ('val_stoi',))
        torch.manual_seed(0)
        ts = TrainStep(net.train(), use_graph=False)
        noise, noisy, clean, _ = stores[0].batch([0, 1], generator=torch.Generator().manual_seed(5))
        ts((noise, noisy, clean, [0, 1]), 0)
        assert getattr(net, '_dcs_skip_flag', None) is None
        second = v.run(EPOCH)
        assert v._graph is not graph                                               # recaptured for the new state key
        fresh = DeviceValidator(net, stores[0], BATCH, seed=SEED, use_graph=False).run(EPOCH)
        _check_losses(second, fresh)
        assert abs(second['val_stoi'] - fresh['val_stoi']) <= 1e-4
        assert second['val_loss'] != first['val_loss']                            # a replay over stale packed weights would repeat it


# ---- 4. validation leaves training alone ------------------------------------------------------------------------------------

def test_fit_with_device_validation_trains_exactly_as_with_host_validation(dev, stores, host_stoi, tmp_path):
    from dcsnet.fit import fit
    val, train = stores
    out = {}
    with _Mode('dcs'):
        for route in ('host', 'device'):
            res = fit(_cnet(dev), train, val, str(tmp_path / route), 2, BATCH, validation=route, log=lambda s: None)
            rows = [json.loads(ln) for ln in open(tmp_path / route / 'metrics.jsonl')]
            out[route] = (res['step'].bucket.flat.detach().clone(), rows)
    (flat_h, rows_h), (flat_d, rows_d) = out['host'], out['device']
    assert torch.equal(flat_h, flat_d)
    assert len(rows_h) == len(rows_d) == 2
    for h, d in zip(rows_h, rows_d):
        assert h['train_loss'] == d['train_loss'] and h['global_step'] == d['global_step'] and h['epoch'] == d['epoch']
        _check_losses(d, h, keys=('val_loss',))
        assert d['val_skipped'] == 0 and 'val_skipped' not in h
        assert d['monitored'] == d['val_loss']


# ---- 5. the real twin, and 'dc' mode ----------------------------------------------------------------------------------------

def test_real_network_device_route_matches_fit_validate(dev, stores, host_stoi):
    from dcsnet.fit import validate
    from dcsnet.validation import DeviceValidator
    with _Mode('drs'):
        net = _rnet(dev)
        host = validate(net, stores[0], BATCH, SEED, EPOCH)
        v = DeviceValidator(net, stores[0], BATCH, seed=SEED, use_graph=False)
        eager = v.run(EPOCH)
    assert list(eager) == list(host)
    assert math.isnan(eager['val_pesq']) and math.isnan(host['val_pesq'])
    assert abs(eager['val_stoi'] - host['val_stoi']) <= 1e-4
    _check_losses(eager, host)
    assert v.counts == {'batches': 3, 'skipped': 0, 'nan_scores': 0}


def test_dc_mode_reports_the_speech_loss_only(dev, stores, host_stoi):
    from dcsnet.fit import validate
    from dcsnet.validation import DeviceValidator
    with _Mode('dc'):
        net = _cnet(dev)
        host = validate(net, stores[0], BATCH, SEED, EPOCH)
        eager = DeviceValidator(net, stores[0], BATCH, seed=SEED, use_graph=False).run(EPOCH)
        test_keys = DeviceValidator(net, stores[0], BATCH, seed=SEED, prefix='test', use_graph=False).run(EPOCH)
    assert set(eager) == set(host) == {'val_speech_loss', 'val_pesq', 'val_stoi'}
    assert set(test_keys) == {'test_speech_loss', 'test_pesq', 'test_stoi'}
    _check_losses(eager, host, keys=('val_speech_loss',))
    assert abs(eager['val_stoi'] - host['val_stoi']) <= 1e-4
    assert test_keys['test_speech_loss'] == eager['val_speech_loss']


def test_bf16_storage_network_device_route_matches_fit_validate(dev, stores, host_stoi):
    """BASELINE configs[4]'s bf16 activation storage (tools/train.py --dtype bf16 --validation device): the same calls."""
    from dcsnet import ops
    from dcsnet.fit import validate
    from dcsnet.validation import DeviceValidator
    default = ops.conv_precision()
    try:
        with _Mode('dcs'):
            net = _cnet(dev).set_activation_dtype('bf16')
            host = validate(net, stores[0], BATCH, SEED, EPOCH)
            v = DeviceValidator(net, stores[0], BATCH, seed=SEED, use_graph=False)
            eager = v.run(EPOCH)
            captured = DeviceValidator(net, stores[0], BATCH, seed=SEED, use_graph=True).run(EPOCH)
    finally:
        ops.set_conv_precision(default)
    assert list(eager) == list(host) == list(captured)
    assert abs(eager['val_stoi'] - host['val_stoi']) <= 1e-4 and abs(captured['val_stoi'] - eager['val_stoi']) <= 1e-4
    _check_losses(eager, host, margin=MARGIN_BF16)
    _check_losses(captured, eager, margin=MARGIN_BF16)
    assert v.counts == {'batches': 3, 'skipped': 0, 'nan_scores': 0}


# ---- 6. extended=True -------------------------------------------------------------------------------------------------------

def test_extended_adds_estoi_and_leaves_stoi_alone(dev, stores, dcs):
    from dcsnet import metrics
    from dcsnet.config import config
    from dcsnet.network_functions import _step
    from dcsnet.validation import DeviceValidator
    net, _, eager, _ = dcs
    with _Mode('dcs'):
        ext = DeviceValidator(net, stores[0], BATCH, seed=SEED, use_graph=False, extended=True).run(EPOCH)
        # the same utterances on the host: the crops of epoch 3, the step's own waveforms, metrics.stoi(extended=True) one by one
        gen = torch.Generator().manual_seed((SEED * 1000003 + EPOCH) & 0x7FFFFFFFFFFFFFFF)
        means = []
        net.eval()
        try:
            with torch.no_grad():
                for idx in stores[0].epoch(BATCH, shuffle=False):
                    noise, noisy, clean, _ = stores[0].batch(idx, generator=gen)
                    a = _step(net, 'complex', noise, noisy, clean, need_noisy_audio=False)
                    c, p = a['clean_audio'].cpu().numpy(), a['predict_clean_audio'].cpu().numpy()
                    vals = [metrics.stoi(c[i], p[i], config.sr, extended=True) for i in range(len(idx))]
                    vals = [v for v in vals if v == v]
                    means.append(sum(vals) / max(len(vals), 1))
        finally:
            net.train()
    want = sum(means) / len(means)
    assert list(ext) == list(eager) + ['val_estoi']
    print(f"val_estoi: {ext['val_estoi']!r} vs {want!r}")
    assert abs(ext['val_estoi'] - want) <= 1e-4
    assert ext['val_stoi'] == eager['val_stoi']                                    # d bit-equal to the default's
    assert all(ext[k] == eager[k] for k in LOSS_KEYS)
