"""Train DCS-Net / DR-Net on a directory of clean / noisy WAV pairs, with checkpoints (dcsnet/fit.py).

    python tools/train.py dcs --clean-dir clean/ --noisy-dir noisy/ --out runs/dcs
    python tools/train.py dcs --clean-dir clean/ --noisy-dir noisy/ --out runs/dcs --resume auto      (continue a stopped run)
    python tools/train.py drs --clean-dir clean/ --noisy-dir noisy/ --out runs/drs --epochs 200 --batch 32
    python tools/train.py dcs --clean-dir clean/ --noisy-dir noisy/ --out runs/dcs --validation device   (validate on the device)
    python tools/train.py dcs --clean-dir clean/ --noise-dir noise/ --out runs/dcs                     (mix on the device)
    python tools/train.py dcs --clean-dir clean/ --noise-dir noise/ --snr-range -5 20 --out runs/dcs

The mode comes first, as in the reference's `train.py dcs 0`: the model code reads it from sys.argv[1].  Files are paired by
name (mono 16-bit PCM at config.file_sr).  With --noise-dir instead of --noisy-dir there are no pairs: every training item is
mixed on the device with a drawn noise recording, noise start and SNR (--snr-db levels, default 15,10,5,0, or --snr-range), by
whole-recording mean powers or, with --level p56 / --noise-level p56, by ITU-T P.56 active speech levels (measured once per store,
on the device); the validation files are mixed once, from a generator seeded by config.seed.  The train / validation split follows the reference's data.py: a seeded shuffle of
the sorted file names, --val-split percent (80) for training; it is written to OUT/partition.json and reused on resume.
OUT receives last.ckpt after every epoch, best.ckpt when the monitored value improved, metrics.jsonl, and final.ckpt — the SWA
weights, the file tools/enhance.py and tools/evaluate.py should load — after the last epoch."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'dcs-net_amd'))

MODES = ('dcs', 'drs', 'dc', 'dr')
LEVELS = ('power', 'p56')                                    # dcsnet.audio_store.LEVELS


def partition(clean_dir, noisy_dir, out_dir, val_split, seed):
    path = os.path.join(out_dir, 'partition.json')
    if os.path.exists(path):
        with open(path) as f:
            return json.load(f)
    import numpy as np
    names = sorted(f for f in os.listdir(noisy_dir) if f.lower().endswith('.wav'))
    if not names:
        raise SystemExit(f'{noisy_dir}: no .wav files')
    missing = [f for f in names if not os.path.isfile(os.path.join(clean_dir, f))]
    if missing:
        raise SystemExit(f'{clean_dir}: no clean file for {missing[0]}' + (f' and {len(missing) - 1} more' if missing[1:] else ''))
    order = np.array(names)
    np.random.RandomState(seed).shuffle(order)
    cut = round(len(order) * (val_split / 100))
    part = {'train': order[:cut].tolist(), 'validation': order[cut:].tolist()}
    if not part['train'] or not part['validation']:
        raise SystemExit(f'{len(names)} files split {val_split} / {100 - val_split} leave an empty set')
    with open(path, 'w') as f:
        json.dump(part, f)
    return part


def _snr_levels(text):
    try:
        levels = [float(v) for v in text.split(',')]
    except ValueError:
        raise argparse.ArgumentTypeError(f'{text!r}: comma-separated dB values expected, as in 15,10,5,0')
    if not levels:
        raise argparse.ArgumentTypeError('at least one SNR level')
    return levels


def parse_args(argv=None):
    """The command line (argv: the arguments after the program name; default sys.argv[1:]); exits on a contradiction."""
    argv = sys.argv[1:] if argv is None else list(argv)
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('mode', choices=MODES, help='dcs / dc: DCS-Net (C_NETWORK); drs / dr: DR-Net (R_NETWORK)')
    ap.add_argument('--clean-dir', required=True)
    ap.add_argument('--noisy-dir', default=None, help='the pre-mixed noisy files, paired with the clean ones by name')
    ap.add_argument('--noise-dir', default=None,
                    help='noise recordings instead of --noisy-dir: every training batch is mixed on the device at drawn SNRs '
                         '(dcsnet.audio_store.MixingAudioStore); the validation part is mixed once, seeded by config.seed')
    ap.add_argument('--snr-db', type=_snr_levels, default=None, help='with --noise-dir: the SNR levels to draw from (15,10,5,0)')
    ap.add_argument('--snr-range', type=float, nargs=2, metavar=('LO', 'HI'), default=None,
                    help='with --noise-dir: a uniform SNR in [LO, HI] dB instead of levels')
    ap.add_argument('--level', default='power', choices=LEVELS,
                    help="with --noise-dir: what the SNR takes as the level of a clean recording: 'power', its whole-recording mean "
                         "square, or 'p56', its ITU-T P.56 active speech level (pauses left out, as VoiceBank+DEMAND was mixed).  A "
                         'property of the store, like --snr-db: a resumed run must be given the same value')
    ap.add_argument('--noise-level', default='power', choices=LEVELS,
                    help='with --noise-dir: the same choice for the noise recordings; a resumed run must be given the same value')
    ap.add_argument('--out', required=True, help='the run directory')
    ap.add_argument('--epochs', type=int, default=None, help='default: config.max_epochs')
    ap.add_argument('--batch', type=int, default=None, help='default: config.batch_size')
    ap.add_argument('--resume', default=None, help="'auto' (OUT/last.ckpt when it exists) or a checkpoint path")
    ap.add_argument('--val-split', type=float, default=80.0, help='percent of the files that train')
    ap.add_argument('--dtype', default='f32', choices=['f32', 'bf16'], help='activation storage (bf16: bf16 MFMA operands)')
    ap.add_argument('--no-graph', action='store_true')
    ap.add_argument('--validation', default='host', choices=['host', 'device'],
                    help="host: net.validation_step per batch (the reference's procedure); device: dcsnet.validation.DeviceValidator "
                         '(losses, STOI and the epoch means on the device, one host read per epoch; val_pesq is NaN)')
    ap.add_argument('--device', default='cuda:0')
    a = ap.parse_args(argv)
    if not argv or argv[0] != a.mode:
        ap.error('the mode must be the first argument (the model code reads sys.argv[1])')
    if (a.noisy_dir is None) == (a.noise_dir is None):
        ap.error('exactly one of --noisy-dir (pre-mixed pairs) and --noise-dir (mix on the device) must be given')
    if a.snr_db is not None and a.snr_range is not None:
        ap.error('--snr-db and --snr-range exclude each other')
    if a.noise_dir is None and (a.snr_db is not None or a.snr_range is not None):
        ap.error('--snr-db / --snr-range need --noise-dir')
    if a.noise_dir is None and (a.level != 'power' or a.noise_level != 'power'):
        ap.error('--level / --noise-level need --noise-dir')
    if a.snr_range is not None and not a.snr_range[0] <= a.snr_range[1]:
        ap.error(f'--snr-range {a.snr_range[0]} {a.snr_range[1]}: LO must not exceed HI')
    if a.mode in ('drs', 'dr') and a.dtype == 'bf16':
        ap.error(f'--dtype bf16 with {a.mode}: the real network has no bf16 activation storage')
    return a


def wav_names(directory):
    names = sorted(f for f in os.listdir(directory) if f.lower().endswith('.wav'))
    if not names:
        raise SystemExit(f'{directory}: no .wav files')
    return names


def main():
    a = parse_args()
    real = a.mode in ('drs', 'dr')
    import torch
    from dcsnet.audio_store import SNR_LEVELS_DB, DeviceAudioStore, MixingAudioStore
    from dcsnet.config import config, hparams
    from dcsnet.fit import fit
    if real:
        from dcsnet.r_network import R_NETWORK as Net
    else:
        from dcsnet.c_network import C_NETWORK as Net
    os.makedirs(a.out, exist_ok=True)
    # --noise-dir: the partition is over the clean files (they pair with themselves)
    part = partition(a.clean_dir, a.noisy_dir or a.clean_dir, a.out, a.val_split, config.seed)
    dev = torch.device(a.device)
    if a.noise_dir is None:
        stores = [DeviceAudioStore.from_wav([os.path.join(a.clean_dir, f) for f in part[k]],
                                            [os.path.join(a.noisy_dir, f) for f in part[k]], config, dev, ids=part[k])
                  for k in ('train', 'validation')]
    else:
        noise = wav_names(a.noise_dir)

        def mixing(k):
            return MixingAudioStore.from_wav([os.path.join(a.clean_dir, f) for f in part[k]],
                                             [os.path.join(a.noise_dir, f) for f in noise], config, dev, ids=part[k],
                                             noise_ids=noise, snr_db=a.snr_db or SNR_LEVELS_DB, snr_range=a.snr_range,
                                             level=a.level, noise_level=a.noise_level)
        # validation is one fixed mixture per file, the same in every run and resume (its noise copy goes with the temporary);
        # training mixes afresh in every batch
        fixed = mixing('validation').materialise(generator=torch.Generator().manual_seed(int(config.seed)))
        stores = [mixing('train'), fixed]
    net = Net(config, dict(hparams), config.seed).to(dev)
    if a.dtype == 'bf16':
        net.set_activation_dtype('bf16')
    out = fit(net, stores[0], stores[1], a.out, a.epochs or config.max_epochs, a.batch or hparams['batch_size'],
              use_graph=not a.no_graph, resume=a.resume, validation=a.validation)
    print(json.dumps({k: v for k, v in out.items() if k not in ('step', 'swa')}))


if __name__ == '__main__':
    main()
