"""What a validation epoch costs by each route (dcsnet/fit.py::validate, dcsnet/validation.py::DeviceValidator): a synthetic store
of --items recordings of about 1 s (256 by default) at batch --batch (32: 8 batches), C_NETWORK in 'dcs' mode, seeded weights.
Per round, each preceded by F.note_state_update() — in fit every validation follows a training epoch, so packed weights and eval
constants are stale and a captured graph's key no longer holds:
  host            fit.validate: the reference's procedure (unfused step, five waveforms to the host, numpy STOI per utterance)
  device_eager    DeviceValidator(use_graph=False).run
  device_graph    DeviceValidator(use_graph=True).run, INCLUDING its two warm passes and the capture (what fit pays per epoch)
and, for scale, device_graph_replay (the same graph again, key still valid: the replays alone) and train_epoch: the same number of
captured TrainStep updates fed by the store.  Host wall clock around work that ends in a device synchronise; the routes alternate
inside a round, so the spread over rounds is this run's run-to-run spread.  The host route is the parent's behaviour: the baseline.
Prints one JSON line and writes it to profiles/validation_bench.json.
usage: python tools/validation_bench.py [--rounds 3 --items 256 --batch 32]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'dcs-net_amd'))


def _store(items, config, dev):
    """Amplitude-modulated tones plus seeded noise, 1.0 to 1.1 s at config.file_sr."""
    from dcsnet.audio_store import DeviceAudioStore
    rng = np.random.default_rng(0)
    sr = int(config.file_sr)
    clean, noisy = [], []
    for i in range(items):
        t = np.arange(int((1.0 + 0.1 * rng.random()) * sr)) / sr
        x = 0.3 * np.sin(2 * np.pi * (150 + 3 * i) * t) * (0.6 + 0.4 * np.sin(2 * np.pi * (2 + i % 7) * t))
        clean.append(x.astype(np.float32))
        noisy.append((x + 0.05 * rng.standard_normal(len(t))).astype(np.float32))
    return DeviceAudioStore(clean, noisy, config, dev)


def _wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--items', type=int, default=256)
    ap.add_argument('--batch', type=int, default=32)
    a = ap.parse_args()
    sys.argv = [sys.argv[0], 'dcs', '0']                         # the model code reads the mode from sys.argv[1]
    from dcsnet import functional as F
    from dcsnet import metrics, network_functions
    from dcsnet.c_network import C_NETWORK
    from dcsnet.config import config, hparams
    from dcsnet.dp import TrainStep
    from dcsnet.fit import validate
    from dcsnet.validation import DeviceValidator
    if not torch.cuda.is_available():
        raise SystemExit('validation_bench: needs a GPU (there is nothing to time without one)')
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    store = _store(a.items, config, dev)
    batches = list(store.epoch(a.batch, shuffle=False))
    net = C_NETWORK(config, dict(hparams), 0).to(dev).train()
    step = TrainStep(net, use_graph=True)
    gen = torch.Generator().manual_seed(1)

    def train_epoch():
        for i, idx in enumerate(batches):
            bufs = step.input_buffers()
            fits = bufs is not None and tuple(bufs[0].shape) == (len(idx), 256, store.T)
            noise, noisy, clean, _ = store.batch(idx, generator=gen, out=bufs if fits else None)
            step((noise, noisy, clean, idx), i)
    train_epoch()                                                 # warm-up: the captures, every shape
    assert step._graph is not None, 'capture did not happen'
    eager, graph = (DeviceValidator(net, store, a.batch, seed=1, use_graph=g) for g in (False, True))
    routes = {'host': lambda: validate(net, store, a.batch, 1, 0), 'device_eager': lambda: eager.run(0),
              'device_graph': lambda: graph.run(0)}
    results = {k: fn() for k, fn in routes.items()}               # warm-up of every route (and the figures to compare)
    rows = {k: [] for k in ('train_epoch', *routes, 'device_graph_replay')}
    for _ in range(a.rounds):
        rows['train_epoch'].append(_wall_ms(train_epoch)[0])
        for name, fn in routes.items():
            F.note_state_update()
            rows[name].append(_wall_ms(fn)[0])
        rows['device_graph_replay'].append(_wall_ms(routes['device_graph'])[0])
    med = {k: round(float(np.median(v)), 2) for k, v in rows.items()}
    spread = {k: round(float(max(v) - min(v)), 2) for k, v in rows.items()}
    line = {'what': 'one validation epoch of C_NETWORK (dcs) by route, ms of host wall clock ending in a device synchronise',
            'items': a.items, 'batch': a.batch, 'batches': len(batches), 'frames': store.T, 'rounds': a.rounds,
            'median_ms': med, 'spread_ms': spread, 'all_ms': {k: [round(x, 2) for x in v] for k, v in rows.items()},
            'host_over_device_eager': round(med['host'] / med['device_eager'], 2),
            'host_over_device_graph': round(med['host'] / med['device_graph'], 2),
            'host_stoi': 'pystoi' if network_functions.stoi is not metrics.stoi else 'dcsnet.metrics.stoi',
            'metrics': {k: {m: (None if v != v else round(v, 6)) for m, v in r.items()} for k, r in results.items()},
            'device': torch.cuda.get_device_name(0)}
    text = json.dumps(line)
    print(text)
    with open(os.path.join(ROOT, 'profiles', 'validation_bench.json'), 'w') as f:
        f.write(text + '\n')


if __name__ == '__main__':
    main()
