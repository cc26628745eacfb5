"""GPU: the training loop with checkpoints (dcsnet/fit.py) on six synthetic recordings — once straight through, once stopped
after its first epoch and resumed — and the files it leaves: last / best / final.ckpt, metrics.jsonl."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPOCHS, BATCH = 3, 2


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from dcsnet import _lib
    _lib.load()
    return torch.device('cuda:0')


def _pairs():
    """Six clean / noisy pairs of 0.6 to 1.0 s at 48 kHz as 16-bit PCM: amplitude-modulated tones plus seeded noise."""
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
def runs(dev, tmp_path_factory):
    from dcsnet.audio_store import DeviceAudioStore
    from dcsnet.config import config, hparams
    from dcsnet.c_network import C_NETWORK
    from dcsnet.fit import fit
    clean, noisy = _pairs()
    train = DeviceAudioStore(clean[:4], noisy[:4], config, dev)
    val = DeviceAudioStore(clean[4:], noisy[4:], config, dev)
    root = tmp_path_factory.mktemp('fit')
    logs = []

    def net():
        return C_NETWORK(config, dict(hparams), 0).to(dev)
    straight = fit(net(), train, val, str(root / 'a'), EPOCHS, BATCH, log=logs.append)
    first = fit(net(), train, val, str(root / 'b'), EPOCHS, BATCH, stop_after_epoch=0, log=logs.append)
    assert not first['finished'] and first['epoch'] == 0 and sorted(os.listdir(root / 'b')) == ['best.ckpt', 'last.ckpt', 'metrics.jsonl']
    resumed = fit(net(), train, val, str(root / 'b'), EPOCHS, BATCH, resume='auto', log=logs.append)
    return root, straight, resumed, noisy, logs


def _lines(path):
    return [json.loads(ln) for ln in open(path)]


def test_a_resumed_run_keeps_the_books_of_an_uninterrupted_one(runs):
    root, a, b, _, logs = runs
    assert a['finished'] and b['finished']
    for k in ('epoch', 'global_step', 'lr', 'scheduler', 'n_averaged'):
        assert a[k] == b[k], k
    assert (a['epoch'], a['global_step'], a['scheduler'], a['n_averaged']) == (EPOCHS - 1, EPOCHS * 2, 'swalr', 2)
    la, lb = _lines(root / 'a' / 'metrics.jsonl'), _lines(root / 'b' / 'metrics.jsonl')
    assert len(la) == len(lb) == EPOCHS and [r['epoch'] for r in lb] == list(range(EPOCHS))
    assert [r['global_step'] for r in la] == [r['global_step'] for r in lb] == [2, 4, 6]
    assert all(np.isfinite(r['train_loss']) and np.isfinite(r['val_loss']) and r['monitored'] == r['val_loss'] for r in la + lb)
    assert la[0]['val_loss'] == pytest.approx(lb[0]['val_loss'], rel=1e-6)      # the first epoch is the same schedule in both
    assert any('resumed' in s for s in logs)
    assert not a['rejected'] and not b['rejected']
    for d in ('a', 'b'):
        assert sorted(os.listdir(root / d)) == ['best.ckpt', 'final.ckpt', 'last.ckpt', 'metrics.jsonl']


def test_final_checkpoint_holds_the_averaged_weights_and_enhances(runs, dev):
    from dcsnet.config import config
    from dcsnet.c_network import C_NETWORK
    from dcsnet.enhance import Enhancer
    root, a, _, noisy, _ = runs
    path = str(root / 'a' / 'final.ckpt')
    net = C_NETWORK.load_from_checkpoint(checkpoint_path=path, config=config, seed=0, map_location='cpu')
    step, swa = a['step'], a['swa']
    assert torch.equal(step.bucket.flat, swa.average)           # on_train_end took the average into the parameters
    live = step.net.state_dict()
    for k, v in net.state_dict().items():
        assert torch.equal(v, live[k].cpu()), k
    enh = Enhancer(net.to(dev).eval(), mode='dcs', segment_frames=64, overlap_frames=16, batch_segments=4, use_graph=False)
    (y,) = enh([torch.from_numpy(noisy[4])], 48000)
    from dcsnet import ops
    assert y.shape == (ops.resample_sinc_length(len(noisy[4]), 48000, 16000),) and bool(torch.isfinite(y).all()) and float(y.abs().max()) > 0


def test_best_and_last_checkpoints_match_the_metrics(runs):
    root, a, _, _, _ = runs
    rows = _lines(root / 'a' / 'metrics.jsonl')
    best = torch.load(str(root / 'a' / 'best.ckpt'), map_location='cpu', weights_only=False)
    last = torch.load(str(root / 'a' / 'last.ckpt'), map_location='cpu', weights_only=False)
    monitored = [r['monitored'] for r in rows]
    assert best['dcsnet']['extra']['monitored'] == min(monitored) == a['best']
    assert best['epoch'] == int(np.argmin(monitored)) and rows[best['epoch']]['improved']
    assert last['epoch'] == EPOCHS - 1 and last['global_step'] == 6
    assert last['dcsnet']['swa']['n_averaged'] == 2 and last['dcsnet']['swa']['scheduler']['kind'] == 'swalr'
    assert last['dcsnet']['counters']['updates'] == 6
