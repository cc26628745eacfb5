"""Trainer-package compatibility: use pytorch_lightning when it is installed (the reference's
runtime, requirements.txt:172); otherwise a minimal stand-in so C_NETWORK is still an nn.Module
with the attributes the reference's step functions touch (self.hparams, self.config, log_dict)."""
import torch

try:                                                       # pragma: no cover - not in this image
    import pytorch_lightning as pl
    try:
        from pytorch_lightning.core.lightning import LightningModule
    except ImportError:
        from pytorch_lightning import LightningModule
    seed_everything = pl.seed_everything
    HAVE_LIGHTNING = True
except ImportError:
    HAVE_LIGHTNING = False

    class LightningModule(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self._hparams = {}
            self.logged = {}

        @property
        def hparams(self):
            return self._hparams

        def save_hyperparameters(self, *args, **kwargs):
            pass

        def log_dict(self, metrics, **kwargs):
            self.logged.update({k: (v.detach() if torch.is_tensor(v) else v) for k, v in metrics.items()})

        @property
        def current_epoch(self):
            return 0

        @classmethod
        def load_from_checkpoint(cls, checkpoint_path, map_location=None, hparams_file=None, **init_kwargs):
            """Lightning's entry as the reference's test.py calls it (test.py:20-26: config=, seed=, checkpoint_path=,
            hparams_file=, map_location=): read a checkpoint in Lightning's layout {'state_dict': ..., 'hyper_parameters':
            ...}, build cls(**init_kwargs), load the state dict strictly, return the module.  `hparams` is the caller's if
            given, else the checkpoint's hyper_parameters (what save_hyperparameters stored: the flat dict, handed to the
            constructor's `hparams` argument as Lightning does), else the project's defaults (config.hparams); keys a
            checkpoint does not hold keep their default.  hparams_file (Lightning's hparams.yaml) replaces the checkpoint's
            hyper-parameters only when a YAML reader is importable; otherwise it is ignored."""
            ckpt = torch.load(checkpoint_path, map_location=map_location, weights_only=False)
            if not isinstance(ckpt, dict) or 'state_dict' not in ckpt:
                raise KeyError(f"{checkpoint_path}: not a Lightning checkpoint (no 'state_dict')")
            if 'hparams' not in init_kwargs:
                from .config import hparams as defaults
                stored = ckpt.get('hyper_parameters') or {}
                if hparams_file is not None:
                    try:
                        import yaml
                    except ImportError:
                        yaml = None
                    if yaml is not None:
                        with open(hparams_file) as f:
                            stored = yaml.safe_load(f) or {}
                stored = dict(stored)
                if set(stored) == {'hparams'} and isinstance(stored['hparams'], dict):
                    stored = dict(stored['hparams'])
                init_kwargs['hparams'] = {**defaults, **stored}
            model = cls(**init_kwargs)
            model.load_state_dict(ckpt['state_dict'], strict=True)
            return model

    def seed_everything(seed):
        import random
        import numpy as np
        random.seed(seed)
        np.random.seed(seed)
        torch.manual_seed(seed)
        return seed
