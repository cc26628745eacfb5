"""CPU-only: load_from_checkpoint of the stand-in LightningModule (dcsnet/_pl_compat.py) as the reference's test.py calls it
(test.py:20-26): Lightning's checkpoint layout in, a module with that state out, strictly."""
import pytest
import torch

from oracle.seeded_state import fill_state, fill_state_stream


def _nets():
    from dcsnet.c_network import C_NETWORK
    from dcsnet.r_network import R_NETWORK
    return {'c': (C_NETWORK, fill_state), 'r': (R_NETWORK, fill_state_stream)}


def _saved(tmp_path, kind, hyper=True, drop=None):
    from dcsnet.config import config, hparams
    cls, fill = _nets()[kind]
    net = fill(cls(config, dict(hparams), 0), 7)
    sd = dict(net.state_dict())
    if drop is not None:
        del sd[drop]
    ckpt = {'state_dict': sd, 'epoch': 3, 'global_step': 1159}
    if hyper:
        # what save_hyperparameters stores: the flat dict (callables excepted here: a checkpoint need not pickle them)
        ckpt['hyper_parameters'] = {k: v for k, v in hparams.items() if not callable(v)}
    path = tmp_path / f'{kind}.ckpt'
    torch.save(ckpt, path)
    return net, str(path)


@pytest.mark.parametrize('kind', ['c', 'r'])
def test_load_from_checkpoint_restores_every_tensor(tmp_path, kind):
    from dcsnet.config import config
    cls = _nets()[kind][0]
    net, path = _saved(tmp_path, kind)
    got = cls.load_from_checkpoint(checkpoint_path=path, config=config, seed=0, hparams_file=None, map_location=None)
    assert type(got) is cls and got.config is config
    want = net.state_dict()
    have = got.state_dict()
    assert list(have) == list(want)
    for k, v in want.items():
        assert have[k].dtype == v.dtype and torch.equal(have[k], v), k


def test_hyper_parameters_come_from_the_caller_then_the_checkpoint_then_the_defaults(tmp_path):
    from dcsnet.config import config, hparams
    from dcsnet.c_network import C_NETWORK
    _, path = _saved(tmp_path, 'c')
    ckpt = torch.load(path, weights_only=False)
    ckpt['hyper_parameters']['speech_alpha'] = 0.25
    torch.save(ckpt, path)
    got = C_NETWORK.load_from_checkpoint(path, config=config, seed=0)
    assert got.hparams['speech_alpha'] == 0.25                                       # the checkpoint's
    assert got.hparams['initialisation_distribution'] is hparams['initialisation_distribution']   # not stored: the default
    mine = dict(hparams, speech_alpha=0.5)
    got = C_NETWORK.load_from_checkpoint(path, config=config, seed=0, hparams=mine)
    assert got.hparams['speech_alpha'] == 0.5                                        # the caller's
    _, bare = _saved(tmp_path, 'c', hyper=False)
    got = C_NETWORK.load_from_checkpoint(bare, config=config, seed=0)
    assert got.hparams['speech_alpha'] == hparams['speech_alpha']                    # the project's defaults


def test_a_file_without_a_state_dict_is_refused(tmp_path):
    from dcsnet.config import config
    from dcsnet.c_network import C_NETWORK
    path = tmp_path / 'bare.ckpt'
    torch.save({'hyper_parameters': {}}, path)
    with pytest.raises(KeyError, match='state_dict'):
        C_NETWORK.load_from_checkpoint(checkpoint_path=str(path), config=config, seed=0)


@pytest.mark.parametrize('kind,key', [('c', 'encoder.2.1.running_covar'), ('r', None)])
def test_a_missing_key_is_refused(tmp_path, kind, key):
    from dcsnet.config import config, hparams
    cls = _nets()[kind][0]
    if key is None:
        key = list(cls(config, dict(hparams), 0).state_dict())[5]
    _, path = _saved(tmp_path, kind, drop=key)
    with pytest.raises(RuntimeError, match='Missing key'):
        cls.load_from_checkpoint(checkpoint_path=path, config=config, seed=0, hparams_file=None, map_location=None)
