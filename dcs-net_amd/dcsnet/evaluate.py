"""How good is an enhanced recording: STOI, SI-SNR and, on request, further groups of measures of whole recordings, scored where
the Enhancer leaves them.

    scorer = RecordingScorer(Enhancer(net, mode='dcs'))          (or a MagnitudeEnhancer)
    scores = scorer.score(noisy_waves, clean_waves, sample_rate=48000)
        -> {'stoi', 'stoi_noisy', 'sisnr', 'sisnr_noisy'}: float32 [n] device tensors; the _noisy entries score the
           unprocessed input against clean, so scores['stoi'] - scores['stoi_noisy'] is what the network gained
    scores, speech = scorer.score(noisy_waves, clean_waves, 48000, return_audio=True)
    scores = scorer.score_files(noisy_paths, clean_paths)         mono 16-bit PCM WAV of one rate

MEASURE_GROUPS below is the one table of what can be scored.  A group is switched on by an attribute of the scorer (extended is
also the constructor's second argument) and adds its measures and their _noisy twins to the dict, behind the groups before it:

    extended            'estoi': the extended STOI (metrics.stoi(..., extended=True)), from the same two STOI calls, each of
                        which then makes both scores in one pass
    frame_measures      'ssnr', 'llr', 'cd': segmental SNR (dB), LPC log-likelihood ratio and LPC cepstrum distance (Hu & Loizou;
                        metrics.frame_measures), at config.sr, from two more calls (metrics.frame_measures_ragged,
                        csrc/frame_measures.hip)
    spectral_measures   'wss', 'fwssnr': weighted spectral slope and frequency-weighted segmental SNR (dB) (Hu & Loizou;
                        metrics.spectral_measures), at config.sr, from two more calls (metrics.spectral_measures_ragged,
                        csrc/spectral_measures.hip)
    sdr                 'sdr': the BSS-eval signal-to-distortion ratio (dB; metrics.sdr, 512 taps), from ONE more call that
                        scores the enhanced and the unprocessed signal against the same clean buffer (metrics.sdr_ragged with
                        estimate2, csrc/sdr_ragged.hip)

The Enhancer keeps everything ragged in one flat device buffer with an int64 offset table; the metrics speak the same
convention (metrics.stoi_ragged / sisnr_ragged, csrc/stoi_ragged.hip), so a whole test set is scored in a handful of launches
and nothing returns to the host before the caller asks for values.  Per call: enhancer.enhance_segments and stitch make the
flat speech estimate; the clean recordings go through the same upload and the same ops.resample_sinc into a store of the
scorer's own, at the plan's offsets; the estimate and the enhancer's resident (resampled) noisy signal are scored against it.
summarise() takes its columns from the dict it is given.  PESQ is not computed; with PESQ values from elsewhere,
metrics.composite_measures gives CSIG / CBAK / COVL (tools/evaluate.py --pesq-csv)."""
from typing import Callable, NamedTuple, Optional

import numpy as np
import torch

from . import metrics
from .audio_store import _signal_shape
from .enhance import Enhancer, read_pcm16


class MeasureGroup(NamedTuple):
    """One group of measures.  switch: the scorer attribute that turns it on (None: always on).  names: its measures, in the
    order of the dict's keys.  lower_is_better: those of them whose improvement is noisy - enhanced.  score: (clean, speech,
    noisy, offsets, sr, longest) -> {key: float32 [n] device tensor} for the group's keys, from flat device buffers at rate sr
    (None: an earlier group's `along` makes them).  along: (a later group's switch, the function to call instead of score while
    that group is on): it returns that group's keys too."""
    switch: Optional[str]
    names: tuple
    lower_is_better: tuple
    score: Optional[Callable]
    along: Optional[tuple] = None

    @property
    def keys(self):
        return tuple(k + side for k in self.names for side in ('', '_noisy'))


def _stoi_sisnr(extended):
    """The two STOI calls (with extended='both': each makes STOI and ESTOI in one pass) and the two SI-SNR calls."""
    def score(clean, speech, noisy, offsets, sr, longest):
        stoi = metrics.stoi_ragged(clean, speech, offsets, sr, longest=longest, extended=extended)
        stoi_noisy = metrics.stoi_ragged(clean, noisy, offsets, sr, longest=longest, extended=extended)
        out = {}
        if extended:
            (stoi, out['estoi']), (stoi_noisy, out['estoi_noisy']) = stoi, stoi_noisy
        out.update(stoi=stoi, stoi_noisy=stoi_noisy, sisnr=metrics.sisnr_ragged(clean, speech, offsets),
                   sisnr_noisy=metrics.sisnr_ragged(clean, noisy, offsets))
        return out
    return score


def _one_call_per_side(ragged):
    """ragged: metrics.frame_measures_ragged or its like, one call -> {name: tensor}."""
    def score(clean, speech, noisy, offsets, sr, longest):
        enhanced = ragged(clean, speech, offsets, sr, longest=longest)
        unprocessed = ragged(clean, noisy, offsets, sr, longest=longest)
        return {**enhanced, **{k + '_noisy': v for k, v in unprocessed.items()}}
    return score


def _sdr(clean, speech, noisy, offsets, sr, longest):
    return dict(zip(('sdr', 'sdr_noisy'), metrics.sdr_ragged(clean, speech, offsets, estimate2=noisy)))


MEASURE_GROUPS = (
    MeasureGroup(None, ('stoi', 'sisnr'), (), _stoi_sisnr(False), along=('extended', _stoi_sisnr('both'))),
    MeasureGroup('extended', ('estoi',), (), None),
    MeasureGroup('frame_measures', ('ssnr', 'llr', 'cd'), ('llr', 'cd'), _one_call_per_side(metrics.frame_measures_ragged)),
    MeasureGroup('spectral_measures', ('wss', 'fwssnr'), ('wss',), _one_call_per_side(metrics.spectral_measures_ragged)),
    MeasureGroup('sdr', ('sdr',), (), _sdr),
)


class RecordingScorer:
    """enhancer: an Enhancer or a MagnitudeEnhancer, used as it is configured (mode, segment geometry, graph).  extended: score
    ESTOI as well.  The other groups of MEASURE_GROUPS are switched on by the attribute of their name (default False; the
    constructor keeps its two arguments).  self.metrics names the dict's keys: those of the groups that are on, in the table's
    order."""

    METRICS, EXTENDED, FRAME_MEASURES, SPECTRAL_MEASURES, SDR = (g.keys for g in MEASURE_GROUPS)

    def __init__(self, enhancer, extended=False):
        if not isinstance(enhancer, Enhancer):
            raise TypeError(f'RecordingScorer: expected an Enhancer or a MagnitudeEnhancer, got {type(enhancer).__name__}')
        self.enhancer = enhancer
        for g in MEASURE_GROUPS[1:]:
            setattr(self, g.switch, False)                   # set it to True on the scorer: the constructor's arguments are pinned
        self.extended = bool(extended)
        self._clean = None                                   # the clean recordings at config.sr, capacity kept across calls

    def _groups(self):
        return [g for g in MEASURE_GROUPS if g.switch is None or getattr(self, g.switch)]

    @property
    def metrics(self):
        return sum((g.keys for g in self._groups()), ())

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
        found = {}
        for g in self._groups():
            fn = g.along[1] if g.along and getattr(self, g.along[0]) else g.score
            if fn is not None:
                found.update(fn(clean, speech, noisy, offsets, enh.sr, longest))
        scores = {k: found[k] for k in self.metrics}
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
    """Host summary of score()'s dict (the one device-to-host transfer) -> (summary dict, per-recording float32 array [n, columns]).
    The columns are METRICS and, behind them in the table's order, the keys of every group of MEASURE_GROUPS whose keys are all in
    the dict.  Per column k the summary has the mean over the recordings that are not NaN and, as k_nan, the count of those that
    are (calc_metric's convention); per measure k it has k_improvement, the mean over the pairs where both sides are numbers
    of enhanced - noisy, or of noisy - enhanced where a lower value is the better one (llr, cd, wss): a positive improvement
    always means the network helped.  A pair of equal infinities (sdr) is left out of that mean like a NaN."""
    groups = [g for g in MEASURE_GROUPS if g.switch is None or all(k in scores for k in g.keys)]
    keys = sum((g.keys for g in groups), ())
    table = torch.stack([scores[k].to(torch.float32) for k in keys], dim=1).cpu().numpy()
    column = dict(zip(keys, table.T))

    def mean(v):
        ok = ~np.isnan(v)
        return float(v[ok].astype(np.float64).sum()) / max(int(ok.sum()), 1)       # calc_metric's mean: NaNs left out

    out = {'files': int(table.shape[0])}
    for k in keys:
        out[k] = mean(column[k])
        out[k + '_nan'] = int(np.isnan(column[k]).sum())
    with np.errstate(invalid='ignore'):                      # inf - inf -> NaN: left out of the mean
        for g in groups:
            for k in g.names:
                enhanced, unprocessed = column[k], column[k + '_noisy']
                out[k + '_improvement'] = mean(unprocessed - enhanced if k in g.lower_is_better else enhanced - unprocessed)
    return out, table
