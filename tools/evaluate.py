"""Score a trained checkpoint on a directory of noisy / clean WAV pairs (dcsnet/evaluate.py): STOI and SI-SNR of the
enhanced and of the unprocessed recordings against the clean ones, on the device.

    python tools/evaluate.py --checkpoint epoch=0-step=289.ckpt noisy_dir/ clean_dir/
    python tools/evaluate.py --checkpoint drs.ckpt --mode drs noisy_dir/ clean_dir/ --csv per_file.csv

Files are paired by name: every *.wav of noisy_dir needs its namesake in clean_dir, mono 16-bit PCM, one sample rate, each pair
of one length.  Prints one JSON line: the file count, the mean of each metric over the files where it is a number (and how
many were not), and the mean improvements stoi - stoi_noisy and sisnr - sisnr_noisy.  --csv writes the per-file table.
--extended adds the extended STOI (ESTOI: estoi, estoi_noisy, estoi_improvement) to the JSON line and the table.
--frame-measures adds segmental SNR, LPC log-likelihood ratio and LPC cepstrum distance (ssnr, llr, cd, their _noisy twins and
ssnr_improvement, llr_improvement, cd_improvement; the last two are noisy - enhanced: lower is better).
--spectral-measures adds the weighted spectral slope and the frequency-weighted segmental SNR (wss, fwssnr, their _noisy twins,
wss_improvement = noisy - enhanced, fwssnr_improvement).
--sdr adds the signal-to-distortion ratio of BSS-eval (mir_eval's bss_eval_sources for one source, 512 taps: sdr, sdr_noisy,
sdr_improvement); beside sisnr it tells filtering from noise, since it forgives a short filter where SI-SNR forgives a gain.
--pesq-csv FILE takes PESQ values computed elsewhere, one line `name,pesq[,pesq_noisy]` per file of the set (name: the WAV
file's name, with or without .wav; '#' lines and a `name,pesq...` header line are skipped), implies --frame-measures and
--spectral-measures, and adds Hu & Loizou's composite measures csig, cbak, covl (metrics.composite_measures) to the JSON line
and the table, with csig_noisy, cbak_noisy, covl_noisy when the third column is there.  A file of the set without a line is
an error."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'dcs-net_amd'))


def pairs(noisy_dir, clean_dir):
    for d in (noisy_dir, clean_dir):
        if not os.path.isdir(d):
            raise SystemExit(f'{d}: not a directory')
    names = sorted(f for f in os.listdir(noisy_dir) if f.lower().endswith('.wav'))
    if not names:
        raise SystemExit(f'{noisy_dir}: no .wav files')
    missing = [f for f in names if not os.path.isfile(os.path.join(clean_dir, f))]
    if missing:
        raise SystemExit(f'{clean_dir}: no clean file for {missing[0]}' + (f' and {len(missing) - 1} more' if missing[1:] else ''))
    return names, [os.path.join(noisy_dir, f) for f in names], [os.path.join(clean_dir, f) for f in names]


def _stem(name):
    return name[:-4] if name.lower().endswith('.wav') else name


def read_pesq_csv(path, names):
    """`name,pesq[,pesq_noisy]` lines -> float64 [len(names), 1 or 2] in the order of names (the set's file names).  Every line
    has the same number of fields; a file of the set that has no line, and a name that has two (with or without .wav), are
    errors that name it."""
    rows, width = {}, None
    with open(path) as f:
        for number, line in enumerate(f, 1):
            fields = [v.strip() for v in line.strip().split(',')]
            if not line.strip() or line.lstrip().startswith('#') or (not rows and fields[1:2] == ['pesq']):
                continue
            if len(fields) not in (2, 3) or (width is not None and len(fields) != width):
                raise SystemExit(f'{path}:{number}: expected name,pesq or name,pesq,pesq_noisy on every line, got {line.strip()!r}')
            width = len(fields)
            if _stem(fields[0]) in rows:
                raise SystemExit(f'{path}:{number}: a second line for {_stem(fields[0])}')
            try:
                rows[_stem(fields[0])] = [float(v) for v in fields[1:]]
            except ValueError:
                raise SystemExit(f'{path}:{number}: not a number in {line.strip()!r}')
    missing = [f for f in names if _stem(f) not in rows]
    if missing:
        raise SystemExit(f'{path}: no PESQ value for {missing[0]}' + (f' and {len(missing) - 1} more' if missing[1:] else ''))
    return np.array([rows[_stem(f)] for f in names], dtype=np.float64).reshape(len(names), -1)


def add_composites(summary, table, keys, pesq):
    """CSIG, CBAK and COVL of every file from its PESQ value(s) pesq [n, 1 or 2] and the llr, wss and ssnr columns of table
    (columns named by keys) -> (summary with their means over the files where they are numbers — NaN where none is —, table with their columns
    appended, keys with their names appended): the enhanced side, then the _noisy side when pesq has a second column."""
    from dcsnet.metrics import composite_measures
    summary, keys, cols = dict(summary), tuple(keys), [table]
    for j, suffix in enumerate(('', '_noisy')[:pesq.shape[1]]):
        col = {k: table[:, keys.index(k + suffix)].astype(np.float64) for k in ('llr', 'wss', 'ssnr')}
        for name, v in composite_measures(pesq[:, j], col['llr'], col['wss'], col['ssnr']).items():
            ok = ~np.isnan(v)
            summary[name + suffix] = float(v[ok].mean()) if ok.any() else float('nan')      # no score is not a score of 0
            summary[name + suffix + '_nan'] = int((~ok).sum())
            cols.append(v[:, None].astype(table.dtype))
            keys = keys + (name + suffix,)
    return summary, np.concatenate(cols, axis=1), keys


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('noisy_dir', help='directory of noisy WAV files')
    ap.add_argument('clean_dir', help='directory of the clean WAV files of the same names')
    ap.add_argument('--checkpoint', required=True)
    ap.add_argument('--hparams-file', default=None, help="Lightning's hparams.yaml (read only when PyYAML is installed)")
    ap.add_argument('--mode', default='dcs', choices=['dcs', 'dc', 'drs', 'dr'],
                    help='dcs / drs: subtract the noise estimate; dc / dr: apply the mask (drs, dr: the real network, R_NETWORK)')
    ap.add_argument('--csv', default=None, help='write the per-file table here')
    ap.add_argument('--extended', action='store_true', help='score the extended STOI (ESTOI) as well')
    ap.add_argument('--frame-measures', action='store_true',
                    help='score segmental SNR, LLR and cepstrum distance (Hu & Loizou) as well')
    ap.add_argument('--spectral-measures', action='store_true',
                    help='score the weighted spectral slope and the frequency-weighted segmental SNR (Hu & Loizou) as well')
    ap.add_argument('--sdr', action='store_true', help='score the BSS-eval signal-to-distortion ratio (512 taps) as well')
    ap.add_argument('--pesq-csv', default=None,
                    help='name,pesq[,pesq_noisy] lines: add CSIG, CBAK and COVL (implies --frame-measures --spectral-measures)')
    ap.add_argument('--segment-frames', type=int, default=2000)
    ap.add_argument('--overlap-frames', type=int, default=300)
    ap.add_argument('--batch-segments', type=int, default=16)
    ap.add_argument('--dtype', default='f32', choices=['f32', 'bf16'], help='activation storage (bf16: bf16 MFMA operands)')
    ap.add_argument('--no-graph', action='store_true')
    ap.add_argument('--device', default='cuda:0')
    a = ap.parse_args()
    real = a.mode in ('drs', 'dr')
    if real and a.dtype == 'bf16':
        ap.error(f'--dtype bf16 with --mode {a.mode}: the real network has no bf16 activation storage')
    names, noisy, clean = pairs(a.noisy_dir, a.clean_dir)
    pesq = None
    if a.pesq_csv:
        pesq = read_pesq_csv(a.pesq_csv, names)
        a.frame_measures = a.spectral_measures = True
    import torch
    from dcsnet.config import config
    from dcsnet.evaluate import MEASURE_GROUPS, RecordingScorer, summarise
    if real:
        from dcsnet.r_network import R_NETWORK as Net
        from dcsnet.enhance import MagnitudeEnhancer as Enh
    else:
        from dcsnet.c_network import C_NETWORK as Net
        from dcsnet.enhance import Enhancer as Enh
    net = Net.load_from_checkpoint(checkpoint_path=a.checkpoint, config=config, seed=config.seed, hparams_file=a.hparams_file,
                                   map_location='cpu')
    net = net.to(torch.device(a.device)).eval()
    if a.dtype == 'bf16':
        net.set_activation_dtype('bf16')
    enh = Enh(net, mode=a.mode, segment_frames=a.segment_frames, overlap_frames=a.overlap_frames,
              batch_segments=a.batch_segments, use_graph=not a.no_graph)
    scorer = RecordingScorer(enh)
    for g in MEASURE_GROUPS[1:]:                             # --frame-measures -> scorer.frame_measures, and so on
        setattr(scorer, g.switch, getattr(a, g.switch))
    summary, table = summarise(scorer.score_files(noisy, clean))
    keys = scorer.metrics
    if pesq is not None:
        summary, table, keys = add_composites(summary, table, keys, pesq)
    if a.csv:
        with open(a.csv, 'w') as f:
            f.write('file,' + ','.join(keys) + '\n')
            for name, row in zip(names, table):
                f.write(name + ',' + ','.join(repr(float(v)) for v in row) + '\n')
    print(json.dumps(dict(summary, mode=a.mode, checkpoint=os.path.basename(a.checkpoint))))


if __name__ == '__main__':
    main()
