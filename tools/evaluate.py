"""Score a trained checkpoint on a directory of noisy / clean WAV pairs (dcsnet/evaluate.py): STOI and SI-SNR of the
enhanced and of the unprocessed recordings against the clean ones, on the device.

    python tools/evaluate.py --checkpoint epoch=0-step=289.ckpt noisy_dir/ clean_dir/
    python tools/evaluate.py --checkpoint drs.ckpt --mode drs noisy_dir/ clean_dir/ --csv per_file.csv

Files are paired by name: every *.wav of noisy_dir needs its namesake in clean_dir, mono 16-bit PCM, one sample rate, each pair
of one length.  Prints one JSON line: the file count, the mean of each metric over the files where it is a number (and how
many were not), and the mean improvements stoi - stoi_noisy and sisnr - sisnr_noisy.  --csv writes the per-file table.
--extended adds the extended STOI (ESTOI: estoi, estoi_noisy, estoi_improvement) to the JSON line and the table.
--frame-measures adds segmental SNR, LPC log-likelihood ratio and LPC cepstrum distance (ssnr, llr, cd, their _noisy twins and
ssnr_improvement, llr_improvement, cd_improvement; the last two are noisy - enhanced: lower is better)."""
import argparse
import json
import os
import sys

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
    import torch
    from dcsnet.config import config
    from dcsnet.evaluate import RecordingScorer, summarise
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
    scorer = RecordingScorer(enh, extended=a.extended)
    scorer.frame_measures = a.frame_measures
    summary, table = summarise(scorer.score_files(noisy, clean))
    if a.csv:
        with open(a.csv, 'w') as f:
            f.write('file,' + ','.join(scorer.metrics) + '\n')
            for name, row in zip(names, table):
                f.write(name + ',' + ','.join(repr(float(v)) for v in row) + '\n')
    print(json.dumps(dict(summary, mode=a.mode, checkpoint=os.path.basename(a.checkpoint))))


if __name__ == '__main__':
    main()
