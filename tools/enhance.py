"""Enhance WAV files with a trained DCS-Net checkpoint (dcsnet/enhance.py).

    python tools/enhance.py --checkpoint epoch=0-step=289.ckpt noisy.wav enhanced.wav
    python tools/enhance.py --checkpoint model.ckpt --mode dc noisy_dir/ enhanced_dir/
    python tools/enhance.py --checkpoint drs.ckpt --mode drs noisy.wav enhanced.wav       (the real twin: drs / dr)

Input: mono 16-bit PCM WAV files of one sample rate (a file, or every *.wav of a directory); output: mono 16-bit PCM at
config.sr under the same names.  The checkpoint is Lightning's layout ({'state_dict', 'hyper_parameters'})."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'dcs-net_amd'))


def paths(src, dst):
    if os.path.isdir(src):
        names = sorted(f for f in os.listdir(src) if f.lower().endswith('.wav'))
        if not names:
            raise SystemExit(f'{src}: no .wav files')
        os.makedirs(dst, exist_ok=True)
        return [os.path.join(src, f) for f in names], [os.path.join(dst, f) for f in names]
    if os.path.isdir(dst):
        dst = os.path.join(dst, os.path.basename(src))
    return [src], [dst]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('input', help='a WAV file or a directory of them')
    ap.add_argument('output', help='the output file or directory')
    ap.add_argument('--checkpoint', required=True)
    ap.add_argument('--hparams-file', default=None, help="Lightning's hparams.yaml (read only when PyYAML is installed)")
    ap.add_argument('--mode', default='dcs', choices=['dcs', 'dc', 'drs', 'dr'],
                    help='dcs / drs: subtract the noise estimate; dc / dr: apply the mask (drs, dr: the real network, R_NETWORK)')
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
    from dcsnet.config import config
    if real:
        from dcsnet.r_network import R_NETWORK as Net
        from dcsnet.enhance import MagnitudeEnhancer as Enh
    else:
        from dcsnet.c_network import C_NETWORK as Net
        from dcsnet.enhance import Enhancer as Enh
    src, dst = paths(a.input, a.output)
    net = Net.load_from_checkpoint(checkpoint_path=a.checkpoint, config=config, seed=config.seed, hparams_file=a.hparams_file,
                                   map_location='cpu')
    net = net.to(torch.device(a.device)).eval()
    if a.dtype == 'bf16':
        net.set_activation_dtype('bf16')
    enh = Enh(net, mode=a.mode, segment_frames=a.segment_frames, overlap_frames=a.overlap_frames,
              batch_segments=a.batch_segments, use_graph=not a.no_graph)
    for p in enh.enhance_files(src, dst):
        print(p)


if __name__ == '__main__':
    main()
