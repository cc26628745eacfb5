"""bench.py's plain run and --dump-outputs: the headline line alone (the --full figures null), and the outputs of the last
timed step written as float32 .npy files that repeat exactly from run to run with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_sample_is_fixed_and_within_the_budget(tmp_path):
    import bench
    x = torch.randn(16, 256, 2000, dtype=torch.complex64, generator=torch.Generator().manual_seed(3))
    small = torch.arange(10, dtype=torch.float64)
    runs = []
    for k in range(2):
        d = tmp_path / f'run{k}'
        info = bench.dump_outputs(str(d), {'mask': x, 'noise_estimate': x.clone(), 'small': small, 'loss': None})
        runs.append({n: np.load(d / f'{n}.npy') for n in info})
        assert sum(os.path.getsize(d / f) for f in os.listdir(d)) <= 64 << 20
    assert info['mask'][0] == [16, 256, 2000, 2] and 0 < info['mask'][1] < x.numel() * 2
    assert info['small'] == ([10], 10) and info['loss'] == ([1], 1)
    for n in runs[0]:
        assert runs[0][n].dtype == np.float32
        np.testing.assert_array_equal(runs[0][n], runs[1][n])
    assert np.isnan(runs[0]['loss']).all()
    np.testing.assert_array_equal(runs[0]['small'], np.arange(10, dtype=np.float32))
    # the sample holds elements of the output itself, in increasing index order
    flat = torch.view_as_real(x).reshape(-1).numpy()
    assert np.isin(runs[0]['mask'][:1000], flat).all()


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['train', 'infer'])
def test_plain_bench_run_dumps_repeatable_outputs(tmp_path, mode):
    lines, dumps = [], []
    for k in range(2):
        d = tmp_path / f'out{k}'
        cmd = [sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '1', '--mode', mode, '--steps', '3', '--warmup', '1',
               '--batch', '2', '--frames', '64', '--dump-outputs', str(d)]
        r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        out = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
        assert len(out) == 1, r.stdout[-500:]
        lines.append(json.loads(out[0]))
        dumps.append({f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))})
    line = lines[0]
    assert line['steps'] == 3 and line['warmup'] == 1 and line['ms_per_step'] > 0 and line['value'] > 0
    assert line['unit'] == 'frames/s' and line['higher_is_better'] is True and line['dtype'] == 'f32'
    assert line['roofline'] is None and line['cpu_baseline'] is None
    assert line['native_f32_mfma'] is None and line['sub_lines'] is None
    names = {'train': {'loss', 'params', 'grads'}, 'infer': {'mask', 'noise_estimate', 'speech_estimate'}}[mode]
    assert set(dumps[0]) == names
    for n in names:
        a, b = dumps[0][n], dumps[1][n]
        assert a.dtype == np.float32 and a.size > 0 and np.isfinite(a).all(), n
        np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-6, err_msg=n)
    # what the timed path computed, not merely something repeatable: the same seeded weights and inputs through the CPU oracle
    import bench
    from dcsnet.config import config, hparams
    from dcsnet.c_network import C_NETWORK
    torch.manual_seed(0)                                     # as bench.py seeds the network it builds
    net = C_NETWORK(config, hparams, 0)
    noise, noisy, clean = bench.synthetic_stft_batch(2, 64, 'cpu', seed=0)
    if mode == 'infer':
        from oracle.cnet_oracle import C_NETWORK_Oracle
        from oracle.nf_oracle import mask_apply_subtract
        oracle = C_NETWORK_Oracle({'dropout_conv': 0.0, 'dropout_fc': 0.0})
        oracle.load_state_dict(net.state_dict(), strict=True)
        with torch.no_grad():
            want = mask_apply_subtract(noisy, oracle.eval()(noisy))
        for n, w, tol in zip(('mask', 'noise_estimate', 'speech_estimate'), want, (2e-4, 6e-4, 6e-4)):
            got = dumps[0][n]
            assert got.shape == (2, 256, 64, 2), (n, got.shape)
            err = float(np.abs(got - torch.view_as_real(w).numpy()).max())
            assert err <= tol, (n, err)
        y = torch.view_as_real(noisy).numpy()
        np.testing.assert_allclose(dumps[0]['noise_estimate'] + dumps[0]['speech_estimate'], y, atol=1e-5)
    else:
        from dcsnet.dp import FlatBucket
        init = FlatBucket(net).flat.numpy()                   # the seeded parameters in the bucket's layout, before any step
        params, grads = dumps[0]['params'], dumps[0]['grads']
        assert params.shape == init.shape == grads.shape and dumps[0]['loss'].size == 1
        # at most 3 eager steps + the captured one + 1 warm-up + 3 timed updates; in its first 8 updates Adam moves an element by
        # at most 1.03 lr per update (Cauchy-Schwarz on |m_hat| / sqrt(v_hat) with b1 = 0.9, b2 = 0.999; AMSGrad only lowers it)
        delta = np.abs(params - init)
        assert 0 < delta.max() <= 1.1 * hparams['lr'] * (4 + 1 + 3), delta.max()
        assert (delta > 0).mean() > 0.5 and (grads != 0).mean() > 0.5
        assert np.abs(grads).max() > 0


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['train', 'infer'])
def test_plain_bench_run_spends_little_time_outside_its_steps(tmp_path, mode):
    """A plain run at the default size (the infer one with --dump-outputs: three 65 MB outputs sampled on the host) may
    spend at most 30 s outside its steps: the whole process's wall time less (steps + warm-up) x ms_per_step."""
    import time
    cmd = [sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '1', '--mode', mode, '--steps', '10', '--warmup', '2']
    if mode == 'infer':
        cmd += ['--dump-outputs', str(tmp_path / 'out')]
    t0 = time.perf_counter()
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=600)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1])
    outside = wall - 12 * line['ms_per_step'] / 1e3
    print(f'{mode}: wall {wall:.2f} s, outside the steps {outside:.2f} s')
    assert outside < 30.0, (wall, line['ms_per_step'])
