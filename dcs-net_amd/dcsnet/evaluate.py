"""How good is an enhanced recording: STOI, SI-SNR and (on request) ESTOI, segmental SNR, LLR, cepstrum distance, WSS,
frequency-weighted segmental SNR and the BSS-eval SDR of whole recordings, scored where the Enhancer leaves them.

    scorer = RecordingScorer(Enhancer(net, mode='dcs'))          (or a MagnitudeEnhancer)
    scores = scorer.score(noisy_waves, clean_waves, sample_rate=48000)
        -> {'stoi', 'stoi_noisy', 'sisnr', 'sisnr_noisy'}: float32 [n] device tensors; the _noisy entries score the
           unprocessed input against clean, so scores['stoi'] - scores['stoi_noisy'] is what the network gained
    scores, speech = scorer.score(noisy_waves, clean_waves, 48000, return_audio=True)
    scores = scorer.score_files(noisy_paths, clean_paths)         mono 16-bit PCM WAV of one rate
    scorer = RecordingScorer(enhancer, extended=True)             the dict gains 'estoi', 'estoi_noisy': the extended STOI
        (ESTOI, metrics.stoi(..., extended=True)), from the same two STOI calls: each makes both scores in one pass
    scorer.frame_measures = True                                  the dict gains 'ssnr', 'llr', 'cd' and their _noisy twins:
        segmental SNR (dB), LPC log-likelihood ratio and LPC cepstrum distance (Hu & Loizou; metrics.frame_measures), at
        config.sr, from two more calls (metrics.frame_measures_ragged, csrc/frame_measures.hip)
    scorer.spectral_measures = True                               the dict gains 'wss', 'fwssnr' and their _noisy twins: weighted
        spectral slope and frequency-weighted segmental SNR (dB) (Hu & Loizou; metrics.spectral_measures), at config.sr, from
        two more calls (metrics.spectral_measures_ragged, csrc/spectral_measures.hip)
    scorer.sdr = True                                             the dict gains 'sdr', 'sdr_noisy': the BSS-eval signal-to-
        distortion ratio (dB; metrics.sdr, 512 taps), from ONE more call that scores the enhanced and the unprocessed signal
        against the same clean buffer (metrics.sdr_ragged with estimate2, csrc/sdr_ragged.hip)

The Enhancer keeps everything ragged in one flat device buffer with an int64 offset table; the metrics speak the same
convention (metrics.stoi_ragged / sisnr_ragged, csrc/stoi_ragged.hip), so a whole test set is scored in a handful of launches
and nothing returns to the host before the caller asks for values.  Per call: enhancer.enhance_segments and stitch make the
flat speech estimate; the clean recordings go through the same upload and the same ops.resample_sinc into a store of the
scorer's own, at the plan's offsets; the estimate and the enhancer's resident (resampled) noisy signal are scored against it.
summarise() takes its columns from the dict it is given.  PESQ is not computed; with PESQ values from elsewhere,
metrics.composite_measures gives CSIG / CBAK / COVL (tools/evaluate.py --pesq-csv)."""
import numpy as np
import torch

from . import metrics
from .audio_store import _signal_shape
from .enhance import Enhancer, read_pcm16


class RecordingScorer:
    """enhancer: an Enhancer or a MagnitudeEnhancer, used as it is configured (mode, segment geometry, graph).  extended: score
    ESTOI as well.  The attribute frame_measures (default False; the constructor keeps its two arguments): score segmental SNR,
    LLR and cepstrum distance as well.  The attribute spectral_measures (default False, likewise): score WSS and the
    frequency-weighted segmental SNR as well.  The attribute sdr (default False, likewise): score the BSS-eval SDR as well.
    self.metrics names the dict's keys: METRICS, then EXTENDED, then FRAME_MEASURES, then SPECTRAL_MEASURES, then SDR where
    asked for."""

    METRICS = ('stoi', 'stoi_noisy', 'sisnr', 'sisnr_noisy')
    EXTENDED = ('estoi', 'estoi_noisy')
    FRAME_MEASURES = ('ssnr', 'ssnr_noisy', 'llr', 'llr_noisy', 'cd', 'cd_noisy')
    SPECTRAL_MEASURES = ('wss', 'wss_noisy', 'fwssnr', 'fwssnr_noisy')
    SDR = ('sdr', 'sdr_noisy')

    def __init__(self, enhancer, extended=False):
        if not isinstance(enhancer, Enhancer):
            raise TypeError(f'RecordingScorer: expected an Enhancer or a MagnitudeEnhancer, got {type(enhancer).__name__}')
        self.enhancer = enhancer
        self.extended = bool(extended)
        self.frame_measures = False                          # set it to True on the scorer: the constructor's arguments are pinned
        self.spectral_measures = False                       # likewise
        self.sdr = False                                     # likewise
        self._clean = None                                   # the clean recordings at config.sr, capacity kept across calls

    @property
    def metrics(self):
        return (self.METRICS + (self.EXTENDED if self.extended else ()) +
                (self.FRAME_MEASURES if self.frame_measures else ()) +
                (self.SPECTRAL_MEASURES if self.spectral_measures else ()) +
                (self.SDR if self.sdr else ()))

    @staticmethod
    def _check_pairs(noisy_waves, clean_waves):
        noisy_waves, clean_waves = list(noisy_waves), list(clean_waves)
        if len(noisy_waves) != len(clean_waves):
            raise ValueError(f'RecordingScorer: {len(noisy_waves)} noisy recordings for {len(clean_waves)} clean ones')
        if not noisy_waves:
            raise ValueError('RecordingScorer: no recordings')
        len_in = np.zeros(len(noisy_waves), dtype=np.int64)
        for i, (a, b) in enumerate(zip(noisy_waves, clean_waves)):
            len_in[i] = _signal_shape(a, f'noisy_waves[{i}]')
            if _signal_shape(b, f'clean_waves[{i}]') != len_in[i]:
                raise ValueError(f'item {i}: clean_data and noisy_data are not the same length '
                                 f'({b.shape[0]} and {a.shape[0]} samples)')
        return noisy_waves, clean_waves, len_in

    def score(self, noisy_waves, clean_waves, sample_rate, return_audio=False):
        """Lists of 1-D float32 / int16 arrays or tensors at sample_rate, pairwise of equal length -> the dict of self.metrics
        (with return_audio: and the list of enhanced recordings, 1-D float32 device tensors at config.sr)."""
        enh = self.enhancer
        noisy_waves, clean_waves, len_in = self._check_pairs(noisy_waves, clean_waves)
        plan, tables, _, segments = enh.enhance_segments(noisy_waves, sample_rate)
        speech = enh.stitch(plan, tables, segments)
        total, offsets = int(plan.offsets[-1]), tables[2]
        if self._clean is None or self._clean.numel() < total:
            self._clean = torch.zeros(max(total, 2 * (0 if self._clean is None else self._clean.numel())), dtype=torch.float32,
                                      device=enh.device)
        enh._resample_into(clean_waves, len_in, int(sample_rate), plan, self._clean, what='clean_waves')
        clean, noisy = self._clean[:total], enh._store[:total]
        longest = int(plan.lengths.max())
        if self.extended:
            stoi, estoi = metrics.stoi_ragged(clean, speech, offsets, enh.sr, longest=longest, extended='both')
            stoi_noisy, estoi_noisy = metrics.stoi_ragged(clean, noisy, offsets, enh.sr, longest=longest, extended='both')
        else:
            stoi = metrics.stoi_ragged(clean, speech, offsets, enh.sr, longest=longest)
            stoi_noisy = metrics.stoi_ragged(clean, noisy, offsets, enh.sr, longest=longest)
        scores = {'stoi': stoi, 'stoi_noisy': stoi_noisy,
                  'sisnr': metrics.sisnr_ragged(clean, speech, offsets),
                  'sisnr_noisy': metrics.sisnr_ragged(clean, noisy, offsets)}
        if self.extended:
            scores['estoi'], scores['estoi_noisy'] = estoi, estoi_noisy
        if self.frame_measures:
            enhanced = metrics.frame_measures_ragged(clean, speech, offsets, enh.sr, longest=longest)
            unprocessed = metrics.frame_measures_ragged(clean, noisy, offsets, enh.sr, longest=longest)
            for k in ('ssnr', 'llr', 'cd'):                  # the order of FRAME_MEASURES
                scores[k], scores[k + '_noisy'] = enhanced[k], unprocessed[k]
        if self.spectral_measures:
            enhanced = metrics.spectral_measures_ragged(clean, speech, offsets, enh.sr, longest=longest)
            unprocessed = metrics.spectral_measures_ragged(clean, noisy, offsets, enh.sr, longest=longest)
            for k in ('wss', 'fwssnr'):                      # the order of SPECTRAL_MEASURES
                scores[k], scores[k + '_noisy'] = enhanced[k], unprocessed[k]
        if self.sdr:
            scores['sdr'], scores['sdr_noisy'] = metrics.sdr_ragged(clean, speech, offsets, estimate2=noisy)
        if return_audio:
            return scores, enh._split(plan, speech)
        return scores

    def score_files(self, noisy_paths, clean_paths, return_audio=False):
        """Mono 16-bit PCM WAV files of one sample rate (scipy.io.wavfile), noisy_paths[i] against clean_paths[i]."""
        noisy_paths, clean_paths = list(noisy_paths), list(clean_paths)
        if len(noisy_paths) != len(clean_paths) or not noisy_paths:
            raise ValueError(f'score_files: {len(noisy_paths)} noisy files for {len(clean_paths)} clean ones')
        noisy, rate = read_pcm16(noisy_paths)
        clean, rate = read_pcm16(clean_paths, rate)
        return self.score(noisy, clean, rate, return_audio=return_audio)


def summarise(scores):
    """Host summary of score()'s dict (the one device-to-host transfer): per metric the mean over the recordings that are not
    NaN and the count of those that are (calc_metric's convention), and the two mean improvements over the pairs where both
    sides are numbers.  -> (summary dict, per-recording float32 array [n, 4] in METRICS order).  With the extended keys in
    the dict ('estoi', 'estoi_noisy'): their columns behind the four, [n, 6], and estoi_improvement in the summary.  With the
    frame-measure keys in the dict (RecordingScorer.FRAME_MEASURES): their six columns behind those, and ssnr_improvement
    (enhanced - noisy, as for the others), llr_improvement and cd_improvement — these two are noisy - enhanced, because a
    lower LLR or cepstrum distance is the better one, so a positive improvement always means the network helped.  With the
    spectral-measure keys in the dict (RecordingScorer.SPECTRAL_MEASURES): their four columns behind those, wss_improvement
    (noisy - enhanced: lower is better) and fwssnr_improvement (enhanced - noisy).  With 'sdr' and 'sdr_noisy' in the dict
    (RecordingScorer.SDR): their two columns behind those and sdr_improvement (enhanced - noisy; a pair of equal
    infinities is left out of its mean like a NaN)."""
    keys = RecordingScorer.METRICS
    extended = all(k in scores for k in RecordingScorer.EXTENDED)
    if extended:
        keys = keys + RecordingScorer.EXTENDED
    measures = all(k in scores for k in RecordingScorer.FRAME_MEASURES)
    if measures:
        keys = keys + RecordingScorer.FRAME_MEASURES
    spectral = all(k in scores for k in RecordingScorer.SPECTRAL_MEASURES)
    if spectral:
        keys = keys + RecordingScorer.SPECTRAL_MEASURES
    sdr = all(k in scores for k in RecordingScorer.SDR)
    if sdr:
        keys = keys + RecordingScorer.SDR
    table = torch.stack([scores[k].to(torch.float32) for k in keys], dim=1).cpu().numpy()

    def mean(v):
        ok = ~np.isnan(v)
        return float(v[ok].astype(np.float64).sum()) / max(int(ok.sum()), 1)       # calc_metric's mean: NaNs left out

    out = {'files': int(table.shape[0])}
    for j, k in enumerate(keys):
        out[k] = mean(table[:, j])
        out[k + '_nan'] = int(np.isnan(table[:, j]).sum())
    out['stoi_improvement'] = mean(table[:, 0] - table[:, 1])
    out['sisnr_improvement'] = mean(table[:, 2] - table[:, 3])
    if extended:
        out['estoi_improvement'] = mean(table[:, 4] - table[:, 5])
    if measures:
        j = keys.index('ssnr')
        out['ssnr_improvement'] = mean(table[:, j] - table[:, j + 1])
        out['llr_improvement'] = mean(table[:, j + 3] - table[:, j + 2])
        out['cd_improvement'] = mean(table[:, j + 5] - table[:, j + 4])
    if spectral:
        j = keys.index('wss')
        out['wss_improvement'] = mean(table[:, j + 1] - table[:, j])
        out['fwssnr_improvement'] = mean(table[:, j + 2] - table[:, j + 3])
    if sdr:
        j = keys.index('sdr')
        with np.errstate(invalid='ignore'):                  # inf - inf -> NaN: left out of the mean
            out['sdr_improvement'] = mean(table[:, j] - table[:, j + 1])
    return out, table
