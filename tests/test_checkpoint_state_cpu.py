"""CPU: the state a training run is continued from (dcsnet/dp.py, dcsnet/swa.py, dcsnet/checkpoint.py) — the optimizer in
torch.optim.Adam's own state_dict format mapped by parameter name, the step's counters, the SWA state, and the checkpoint file
in Lightning 1.5.6's layout.  The optimizer that steps here is the torch reference (TorchAdam); FusedAdam is built on CPU
buckets only to import and export (its step needs the device: tests/test_resume_gpu.py)."""
import copy
import ctypes
import os

import pytest
import torch


class _Lstm(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.real_lstm = torch.nn.LSTM(4, 4, bidirectional=True)
        self.imag_lstm = torch.nn.LSTM(4, 4, bidirectional=True)


class _Toy(torch.nn.Module):
    """tests/test_swa_gpu.py's _Toy (sizes that are no multiples of 4: padded slices), a ComplexLSTM-like pair (the bucket puts
    its groups first: bucket order != registration order) and a parameter that never gets a gradient, under a name the
    bucket leaves out as the reference's optimizer leaves it without state."""

    def __init__(self, seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.a = torch.nn.Parameter(torch.randn(37, 5, generator=g))
        self.b = torch.nn.Parameter(torch.randn(1001, generator=g))
        self.c = torch.nn.Parameter(torch.randn(3, generator=g))
        torch.manual_seed(seed)
        self.lstm = _Lstm()
        self.decoder_attention = torch.nn.ModuleDict({'12': torch.nn.Linear(3, 2)})


KW = dict(lr=1e-2, eps=1e-6, weight_decay=1e-3)


def _trained_adam_state(steps=3):
    toy = _Toy()
    opt = torch.optim.Adam(toy.parameters(), amsgrad=True, **KW)
    g = torch.Generator().manual_seed(5)
    for _ in range(steps):
        for n, p in toy.named_parameters():
            p.grad = None if n.startswith('decoder_attention') else torch.randn(p.shape, generator=g)
        opt.step()
    return toy, copy.deepcopy(opt.state_dict())


def _same_adam_state(got, want):
    assert list(got['state']) == list(want['state'])
    for k, e in want['state'].items():
        assert set(got['state'][k]) == set(e), k
        for f, v in e.items():
            assert torch.equal(torch.as_tensor(got['state'][k][f]), torch.as_tensor(v)), (k, f)
            assert torch.as_tensor(got['state'][k][f]).dtype == torch.as_tensor(v).dtype, (k, f)
    assert got['param_groups'] == want['param_groups']


@pytest.mark.parametrize('fused', [False, True])
def test_adam_state_round_trip_by_name(fused):
    from dcsnet.dp import FlatBucket, TorchAdam, FusedAdam
    toy, sd0 = _trained_adam_state()
    names = [n for n, _ in toy.named_parameters()]
    absent = [i for i, n in enumerate(names) if n.startswith('decoder_attention')]
    assert len(absent) == 2 and all(i not in sd0['state'] for i in absent) and len(sd0['state']) == len(names) - 2
    twin = _Toy(seed=9)
    bucket = FlatBucket(twin)
    assert bucket.names != [n for n in names if not n.startswith('decoder_attention')], 'the bucket must reorder'
    assert bucket.numel > sum(p.numel() for p in bucket.params), 'slices must be padded'
    opt = (FusedAdam if fused else TorchAdam)(bucket, **KW)
    opt.load_state_dict(copy.deepcopy(sd0))
    sd1 = opt.state_dict()
    _same_adam_state(sd1, sd0)
    assert sd1['param_groups'][0]['params'] == list(range(len(names)))
    if fused:
        assert int(opt.t_dev) == 3 and opt.t == 3
        covered = torch.zeros(bucket.numel, dtype=torch.bool)
        for o, p in zip(bucket.offsets, bucket.params):
            covered[o:o + p.numel()] = True
        for buf in (opt.m, opt.v, opt.vmax):
            assert not buf[~covered].any()
    # a stock optimizer accepts the export
    stock = torch.optim.Adam(_Toy(seed=4).parameters(), amsgrad=True, **KW)
    stock.load_state_dict(sd1)
    _same_adam_state(stock.state_dict(), sd0)


def test_adam_state_accepts_integer_steps_and_takes_the_rate():
    """torch 1.10 (the reference's era) stored `step` as a Python int; lr comes from the loaded group."""
    from dcsnet.dp import FlatBucket, FusedAdam
    _, sd = _trained_adam_state()
    for e in sd['state'].values():
        e['step'] = 3
    sd['param_groups'][0]['lr'] = 2.5e-3
    opt = FusedAdam(FlatBucket(_Toy(seed=1)), **KW)
    opt.load_state_dict(sd)
    assert int(opt.t_dev) == 3 and opt.lr == 2.5e-3
    assert opt._lr_dev_value != 2.5e-3          # the next sync_lr() writes it to the device scalar


def test_adam_state_refusals_name_the_field():
    from dcsnet.dp import FlatBucket, FusedAdam, TorchAdam
    for cls in (FusedAdam, TorchAdam):
        opt = cls(FlatBucket(_Toy(seed=1)), **KW)
        _, sd = _trained_adam_state()
        first = next(iter(sd['state']))
        bad = copy.deepcopy(sd)
        bad['state'][first]['step'] = torch.tensor(7.0)
        with pytest.raises(ValueError, match='step'):
            opt.load_state_dict(bad)
        bad = copy.deepcopy(sd)
        for e in bad['state'].values():
            del e['max_exp_avg_sq']
        bad['param_groups'][0]['amsgrad'] = False
        with pytest.raises(ValueError, match='max_exp_avg_sq'):
            opt.load_state_dict(bad)
        bad = copy.deepcopy(sd)
        del bad['state'][first]['max_exp_avg_sq']
        with pytest.raises(ValueError, match='max_exp_avg_sq'):
            opt.load_state_dict(bad)
        bad = copy.deepcopy(sd)
        bad['param_groups'][0]['eps'] = 1e-8
        with pytest.raises(ValueError, match='eps'):
            opt.load_state_dict(bad)
        bad = copy.deepcopy(sd)
        bad['param_groups'][0]['betas'] = (0.8, 0.999)
        with pytest.raises(ValueError, match='betas'):
            opt.load_state_dict(bad)
        bad = copy.deepcopy(sd)
        bad['param_groups'][0]['weight_decay'] = 0.0
        with pytest.raises(ValueError, match='weight_decay'):
            opt.load_state_dict(bad)
        opt.load_state_dict(sd)                 # and the untouched one loads


def test_name_mapping_on_c_network():
    """A seeded fake Adam state per net.parameters() index: after the import every hot parameter's slice of m / v / vmax is
    the tensor stored under its NAME, the padding is zero, and decoder_attention.12/13 were ignored."""
    from dcsnet.config import config, hparams
    from dcsnet.c_network import C_NETWORK
    from dcsnet.dp import FlatBucket, FusedAdam, UNUSED_PREFIXES
    net = C_NETWORK(config, dict(hparams), 0)
    named = list(net.named_parameters())
    state = {}
    for i, (n, p) in enumerate(named):
        g = torch.Generator().manual_seed(1000 + i)
        state[i] = {'step': torch.tensor(5.0), 'exp_avg': torch.randn(p.shape, generator=g),
                    'exp_avg_sq': torch.rand(p.shape, generator=g), 'max_exp_avg_sq': torch.rand(p.shape, generator=g) + 1}
    sd = {'state': state, 'param_groups': [dict(lr=1e-4, betas=(0.9, 0.999), eps=1e-6, weight_decay=1e-4, amsgrad=True,
                                                params=list(range(len(named))))]}
    bucket = FlatBucket(net)
    opt = FusedAdam(bucket, lr=1e-4, eps=1e-6, weight_decay=1e-4)
    opt.load_state_dict(sd)
    index = {n: i for i, (n, _) in enumerate(named)}
    assert any(n.startswith(UNUSED_PREFIXES) for n in index) and not any(n.startswith(UNUSED_PREFIXES) for n in bucket.names)
    assert bucket.names[0].startswith('lstm.') and named[0][0] != bucket.names[0]
    covered = torch.zeros(bucket.numel, dtype=torch.bool)
    for n, o, p in zip(bucket.names, bucket.offsets, bucket.params):
        for f, buf in (('exp_avg', opt.m), ('exp_avg_sq', opt.v), ('max_exp_avg_sq', opt.vmax)):
            assert torch.equal(buf[o:o + p.numel()], state[index[n]][f].reshape(-1)), (n, f)
        covered[o:o + p.numel()] = True
    assert int((~covered).sum()) == bucket.numel - sum(p.numel() for p in bucket.params) > 0
    for buf in (opt.m, opt.v, opt.vmax):
        assert not buf[~covered].any()
    assert int(opt.t_dev) == 5
    out = opt.state_dict()
    assert sorted(out['state']) == sorted(index[n] for n in bucket.names)


# ---- the checkpoint file -------------------------------------------------------------------------------------------------

class _OracleAdapter(torch.nn.Module):
    """tests/test_dp_cpu.py's adapter — the CPU oracle under C_NETWORK's parameter names with the attributes TrainStep touches —
    which also hands out the oracle's own state_dict, so that the file is the one C_NETWORK.load_from_checkpoint reads."""

    def __init__(self, seed):
        super().__init__()
        from oracle.cnet_oracle import C_NETWORK_Oracle
        from oracle.seeded_state import fill_state
        self.net = fill_state(C_NETWORK_Oracle({'dropout_conv': 0.0, 'dropout_fc': 0.0}), seed)
        self.hparams = {'lr': 1e-4, 'optim_eps': 1e-6, 'optim_weight_decay': 1e-4, 'gradient_clip_val': 100.0}

    def named_parameters(self, *a, **k):
        return self.net.named_parameters(*a, **k)

    def state_dict(self, *a, **k):
        return self.net.state_dict(*a, **k)

    def load_state_dict(self, *a, **k):
        return self.net.load_state_dict(*a, **k)

    def training_step(self, batch, idx):
        from oracle.nf_oracle import dcs_train_losses
        noise, noisy, clean = batch[:3]
        return dcs_train_losses(self.net, noise, noisy, clean)[2]


def _batch(seed, B=1, T=16):
    from oracle.seeded_state import seeded_input
    clean, noise = seeded_input(B, 256, T, 10 + seed, 0.1), seeded_input(B, 256, T, 20 + seed, 0.05)
    return noise, clean + noise, clean


def _driver(seed, max_epochs=4):
    from dcsnet.dp import TrainStep, TorchAdam, plateau_scheduler
    from dcsnet.swa import StochasticWeightAveraging
    step = TrainStep(_OracleAdapter(seed), optimizer_cls=TorchAdam)
    swa = StochasticWeightAveraging(step, max_epochs, swa_epoch_start=0.5, lr_scheduler=plateau_scheduler(step.optimizer))
    return step, swa


@pytest.fixture(scope='module')
def saved(tmp_path_factory):
    """One driver run past the SWA start (epochs 0-2 of 4, one step each; swa_start = 1), saved after epoch 2."""
    from dcsnet.checkpoint import save_checkpoint
    torch.manual_seed(11)
    step, swa = _driver(seed=3)
    for epoch in range(3):
        swa.on_train_epoch_start(epoch)
        step(_batch(epoch))
        swa.on_train_epoch_end(epoch, monitored=1.0 / (epoch + 1))
    gen = torch.Generator().manual_seed(77)
    torch.rand(5, generator=gen)
    path = str(tmp_path_factory.mktemp('ckpt') / 'last.ckpt')
    save_checkpoint(path, step, swa, epoch=2, global_step=3, generator=gen, extra={'best': 0.5})
    at_save = {'flat': step.bucket.flat.clone(), 'net': {k: v.clone() for k, v in step.net.state_dict().items()},
               'step': step.state_dict(), 'average': swa.average.clone(), 'scheduler': copy.deepcopy(swa.lr_scheduler.state_dict()),
               'scheduler_type': type(swa.lr_scheduler), 'lr': step.optimizer.param_groups[0]['lr'], 'generator': gen.get_state().clone()}
    swa.on_train_epoch_start(3)                              # the uninterrupted run goes on: what a resumed one must reproduce
    step(_batch(3))
    at_save['later'] = (step.bucket.flat.clone(), swa.average.clone())
    return path, step, at_save, gen


def test_checkpoint_file_has_lightnings_layout_and_load_from_checkpoint_reads_it(saved):
    from dcsnet.config import config
    from dcsnet.c_network import C_NETWORK
    path, step, at_save, _ = saved
    ckpt = torch.load(path, map_location='cpu', weights_only=False)
    assert set(ckpt) == {'epoch', 'global_step', 'pytorch-lightning_version', 'state_dict', 'optimizer_states', 'lr_schedulers',
                         'callbacks', 'hyper_parameters', 'dcsnet'}
    assert (ckpt['epoch'], ckpt['global_step'], ckpt['pytorch-lightning_version'], ckpt['callbacks']) == (2, 3, '1.5.6', {})
    assert len(ckpt['optimizer_states']) == 1 and len(ckpt['lr_schedulers']) == 1
    assert ckpt['hyper_parameters'] == step.net.hparams
    own = ckpt['dcsnet']
    assert own['format'] == 1 and own['mode'] == 'dcs' and own['extra'] == {'best': 0.5}
    assert own['counters']['calls'] == own['counters']['updates'] == 3
    assert own['swa']['n_averaged'] == 2 and own['swa']['scheduler']['kind'] == 'swalr'
    assert set(own['swa']['average']) == set(step.bucket.names)
    net = C_NETWORK.load_from_checkpoint(checkpoint_path=path, config=config, seed=0, map_location='cpu')
    for k, v in net.state_dict().items():
        assert torch.equal(v, at_save['net'][k]), k


def test_checkpoint_restores_a_differently_seeded_step(saved):
    from dcsnet.checkpoint import load_checkpoint
    path, _, want, _ = saved
    torch.manual_seed(11)
    step2, swa2 = _driver(seed=8)
    step2(_batch(5))                                        # its own state first: moments, counters
    flat_ptr, avg_ptr = step2.bucket.flat.data_ptr(), swa2.average.data_ptr()
    assert not torch.equal(step2.bucket.flat, want['flat'])
    gen2 = torch.Generator().manual_seed(1)
    got = load_checkpoint(path, step2, swa2, generator=gen2)
    assert got == {'epoch': 2, 'global_step': 3, 'extra': {'best': 0.5}}
    assert (step2.bucket.flat.data_ptr(), swa2.average.data_ptr()) == (flat_ptr, avg_ptr)        # in place
    assert torch.equal(step2.bucket.flat, want['flat'])
    a, b = want['net'], step2.net.state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    sa, sb = want['step'], step2.state_dict()
    assert sa['counters'] == sb['counters'] and sb['counters']['updates'] == 3
    assert list(sa['optimizer']['state']) == list(sb['optimizer']['state'])
    for k, e in sa['optimizer']['state'].items():
        for f, v in e.items():
            assert torch.equal(v, sb['optimizer']['state'][k][f]), (k, f)
    assert sa['optimizer']['param_groups'] == sb['optimizer']['param_groups']
    assert swa2.n_averaged == 2 and torch.equal(swa2.average, want['average'])
    assert type(swa2.lr_scheduler) is want['scheduler_type']
    assert swa2.lr_scheduler.state_dict() == want['scheduler']
    assert step2.optimizer.param_groups[0]['lr'] == want['lr']
    assert torch.equal(gen2.get_state(), want['generator'])
    # and it continues as the uninterrupted run did: one more epoch start (an average update) and step
    swa2.on_train_epoch_start(3)
    step2(_batch(3))
    assert torch.equal(step2.bucket.flat, want['later'][0]) and torch.equal(swa2.average, want['later'][1])


def test_reference_style_checkpoint_loads_with_updates_from_the_optimizer(saved, tmp_path):
    """A file without the project's key — what the reference's own training writes — restores weights, optimizer, scheduler
    and epoch; the counters become updates = step, seed_state = 0."""
    from dcsnet.checkpoint import load_checkpoint
    from dcsnet.dp import TrainStep, TorchAdam, plateau_scheduler
    from dcsnet.swa import StochasticWeightAveraging
    path, step, _, _ = saved
    ckpt = torch.load(path, map_location='cpu', weights_only=False)
    del ckpt['dcsnet']
    plateau = plateau_scheduler(torch.optim.Adam([torch.zeros(1, requires_grad=True)], lr=1e-4))
    for v in (3.0, 2.0, 2.5):
        plateau.step(v)
    ckpt['lr_schedulers'] = [plateau.state_dict()]
    ref = str(tmp_path / 'reference.ckpt')
    torch.save(ckpt, ref)
    step2 = TrainStep(_OracleAdapter(8), optimizer_cls=TorchAdam)
    swa2 = StochasticWeightAveraging(step2, 200, lr_scheduler=plateau_scheduler(step2.optimizer))
    got = load_checkpoint(ref, step2, swa2)
    assert got == {'epoch': 2, 'global_step': 3, 'extra': None}
    c = step2.state_dict()['counters']
    assert c['updates'] == 3 and c['calls'] == 3 and c['seed_state'] == 0
    live = step2.net.state_dict()
    assert all(torch.equal(live[k], v) for k, v in ckpt['state_dict'].items())
    assert swa2.lr_scheduler.best == 2.0 and swa2.lr_scheduler.num_bad_epochs == 1 and swa2.lr_scheduler.last_epoch == 3


def test_checkpoint_refuses_a_foreign_mode_and_foreign_names(saved, tmp_path):
    from dcsnet.checkpoint import load_checkpoint
    path, _, _, _ = saved
    step2, swa2 = _driver(seed=8)
    ckpt = torch.load(path, map_location='cpu', weights_only=False)
    ckpt['dcsnet']['mode'] = 'dc'
    torch.save(ckpt, str(tmp_path / 'mode.ckpt'))
    with pytest.raises(ValueError, match='mode'):
        load_checkpoint(str(tmp_path / 'mode.ckpt'), step2, swa2)
    ckpt['dcsnet']['mode'] = 'dcs'
    ckpt['dcsnet']['activation_dtype'] = 'torch.bfloat16'
    torch.save(ckpt, str(tmp_path / 'dtype.ckpt'))
    with pytest.raises(ValueError, match='activation_dtype'):
        load_checkpoint(str(tmp_path / 'dtype.ckpt'), step2, swa2)
    ckpt['dcsnet']['activation_dtype'] = 'torch.float32'
    ckpt['state_dict']['encoder.0.0.extra'] = torch.zeros(1)
    torch.save(ckpt, str(tmp_path / 'names.ckpt'))
    with pytest.raises(ValueError, match='names'):
        load_checkpoint(str(tmp_path / 'names.ckpt'), step2, swa2)


def test_a_nan_moment_is_never_written(saved, tmp_path):
    from dcsnet.checkpoint import save_checkpoint, load_checkpoint, NonFiniteState
    path, _, _, _ = saved
    step2, swa2 = _driver(seed=8)
    load_checkpoint(path, step2, swa2)
    out = str(tmp_path / 'last.ckpt')
    save_checkpoint(out, step2, swa2, epoch=2, global_step=3)
    before = open(out, 'rb').read()
    p = step2.bucket.params[3]
    step2.opt.opt.state[p]['exp_avg_sq'].view(-1)[0] = float('nan')
    with pytest.raises(NonFiniteState, match='exp_avg_sq') as ei:
        save_checkpoint(out, step2, swa2, epoch=3, global_step=4)
    assert list(ei.value.counts.values()) == [1]
    assert open(out, 'rb').read() == before
    assert sorted(os.listdir(tmp_path)) == ['last.ckpt']                  # no temporary file left behind


def test_train_step_warns_when_the_dropout_seed_differs(saved):
    from dcsnet.checkpoint import load_checkpoint
    path, _, _, _ = saved
    step2, swa2 = _driver(seed=8)
    torch.manual_seed(12)
    with pytest.warns(UserWarning, match='initial_seed'):
        load_checkpoint(path, step2, swa2)
    torch.manual_seed(11)


# ---- C ABI ---------------------------------------------------------------------------------------------------------------

def test_snapshot_entry_point_is_exported_and_checks_its_arguments_without_a_gpu():
    from dcsnet import _lib
    lib = _lib.load()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), 'dcs_snapshot_words')
    assert lib.dcs_abi_version() == 20                       # new entry points only: no signature changed
    assert ctypes.sizeof(_lib.SnapshotItem) == 32
    items, first = (_lib.SnapshotItem * 2)(), (ctypes.c_long * 3)()
    dst, cnt = ctypes.create_string_buffer(64 + 16), (ctypes.c_int * 2)()
    d = (ctypes.addressof(dst) + 15) & ~15
    ok = [ctypes.addressof(items), 1, ctypes.addressof(first), d, 16, ctypes.addressof(cnt), None]
    for i in (0, 2, 3, 5):
        bad = list(ok)
        bad[i] = None
        assert lib.dcs_snapshot_words(*bad) == -1, i
    for n in (0, -1, 1025):
        assert lib.dcs_snapshot_words(ok[0], n, *ok[2:]) == -1, n
    assert lib.dcs_snapshot_words(ok[0], 1, ok[2], d, -1, ok[5], None) == -1          # negative size
    assert lib.dcs_snapshot_words(ok[0], 1, ok[2], d + 4, 16, ok[5], None) == -1      # a slab that is not 16-byte aligned


def test_snapshot_wrappers_refuse_cpu_tensors():
    from dcsnet import ops, DcsHipError
    with pytest.raises(DcsHipError, match='no CPU fallback'):
        ops.snapshot_table([torch.zeros(8)])
    with pytest.raises(DcsHipError):
        ops.snapshot_table([])
