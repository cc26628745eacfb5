"""Mix a directory of clean speech with a directory of noise recordings into a fixed test set, on the device
(dcsnet.audio_store.MixingAudioStore.materialise: one mixture per clean file).

    python tools/mix.py clean_dir/ noise_dir/ --out testset/
    python tools/mix.py clean_dir/ noise_dir/ --out testset/ --snr-db 17.5,12.5,7.5,2.5 --seed 3
    python tools/evaluate.py --checkpoint final.ckpt testset/noisy testset/clean

Input: mono 16-bit PCM WAV at config.file_sr.  Per clean file a noise recording, a noise start and an SNR are drawn from a
generator seeded by --seed (default config.seed); the noise loops from its start and is scaled by whole-recording mean powers, or
with --level p56 / --noise-level p56 by ITU-T P.56 active speech levels (measured on the device).  OUT/noisy/NAME and OUT/clean/NAME are written as mono 16-bit PCM at config.sr (the clean
file resampled, so every pair has one rate and one length: what tools/evaluate.py reads), and OUT/draws.csv holds one line per
file: name, noise file, noise start (samples at config.sr), SNR in dB, gain, clipped-sample count of the mixture.  The conversion
to PCM (x 32768, nearest, clipped to +-32767) runs on the host."""
import argparse
import csv
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'dcs-net_amd'))


LEVELS = ('power', 'p56')                                    # dcsnet.audio_store.LEVELS


def wav_names(directory):
    if not os.path.isdir(directory):
        raise SystemExit(f'{directory}: not a directory')
    names = sorted(f for f in os.listdir(directory) if f.lower().endswith('.wav'))
    if not names:
        raise SystemExit(f'{directory}: no .wav files')
    return names


def to_pcm16(x):
    """float32 samples -> (int16 samples: x 32768, rounded to nearest even, clipped to +-32767; how many were clipped)."""
    v = np.rint(np.asarray(x, dtype=np.float64) * 32768.0)
    clipped = int(np.count_nonzero(np.abs(v) > 32767))
    return np.clip(v, -32767, 32767).astype(np.int16), clipped


def _snr_levels(text):
    try:
        return [float(v) for v in text.split(',')]
    except ValueError:
        raise argparse.ArgumentTypeError(f'{text!r}: comma-separated dB values expected, as in 15,10,5,0')


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('clean_dir')
    ap.add_argument('noise_dir')
    ap.add_argument('--out', required=True, help='receives noisy/, clean/ and draws.csv')
    ap.add_argument('--snr-db', type=_snr_levels, default=None, help='the SNR levels to draw from (default 15,10,5,0)')
    ap.add_argument('--snr-range', type=float, nargs=2, metavar=('LO', 'HI'), default=None, help='a uniform SNR in [LO, HI] dB')
    ap.add_argument('--level', default='power', choices=LEVELS,
                    help="what the SNR takes as the level of a clean recording: 'power', its whole-recording mean square, or 'p56', its "
                         'ITU-T P.56 active speech level (pauses left out, as VoiceBank+DEMAND was mixed)')
    ap.add_argument('--noise-level', default='power', choices=LEVELS, help='the same choice for the noise recordings')
    ap.add_argument('--seed', type=int, default=None, help='default: config.seed')
    ap.add_argument('--device', default='cuda:0')
    a = ap.parse_args(argv)
    if a.snr_db is not None and a.snr_range is not None:
        ap.error('--snr-db and --snr-range exclude each other')
    return a


def main():
    a = parse_args()
    clean_names, noise_names = wav_names(a.clean_dir), wav_names(a.noise_dir)
    import torch
    from scipy.io import wavfile
    from dcsnet.audio_store import SNR_LEVELS_DB, MixingAudioStore
    from dcsnet.config import config
    store = MixingAudioStore.from_wav([os.path.join(a.clean_dir, f) for f in clean_names],
                                      [os.path.join(a.noise_dir, f) for f in noise_names], config, torch.device(a.device),
                                      ids=clean_names, noise_ids=noise_names, snr_db=a.snr_db or SNR_LEVELS_DB,
                                      snr_range=a.snr_range, level=a.level, noise_level=a.noise_level)
    fixed = store.materialise(generator=torch.Generator().manual_seed(int(config.seed if a.seed is None else a.seed)))
    draws = store.last_draws
    clean, noisy = fixed.clean.cpu().numpy(), fixed.noisy.cpu().numpy()
    off = np.concatenate([[0], np.cumsum(fixed.lengths)])
    for d in ('noisy', 'clean'):
        os.makedirs(os.path.join(a.out, d), exist_ok=True)
    with open(os.path.join(a.out, 'draws.csv'), 'w', newline='') as f:
        rows = csv.writer(f)
        rows.writerow(['name', 'noise_file', 'noise_start', 'snr_db', 'gain', 'clipped_samples'])
        for i, name in enumerate(clean_names):
            pcm, clipped = to_pcm16(noisy[off[i]:off[i + 1]])
            wavfile.write(os.path.join(a.out, 'noisy', name), int(config.sr), pcm)
            wavfile.write(os.path.join(a.out, 'clean', name), int(config.sr), to_pcm16(clean[off[i]:off[i + 1]])[0])
            rows.writerow([name, noise_names[draws['noise_index'][i]], draws['noise_start'][i], repr(draws['snr_db'][i]),
                           repr(float(draws['gain'][i])), clipped])
    print(f'{len(clean_names)} mixtures at {config.sr} Hz in {a.out} ({os.path.join(a.out, "draws.csv")})')


if __name__ == '__main__':
    main()
