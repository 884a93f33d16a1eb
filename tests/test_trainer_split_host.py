"""hipets.ModelTrainer(step_kernel=...) on the host: which kernel a batch size is sent to, over a recording CPU engine."""
import numpy as np
import pytest
import torch

import hipets
import train_restatement as tr


class _Recorder(tr.CpuEngine):
    def train_steps(self, *a, **kw):
        self.kernels = getattr(self, "kernels", []) + [kw.pop("kernel", None)]
        return super().train_steps(*a, **kw)


@pytest.mark.parametrize("step_kernel, batch_size, sent", [("auto", 256, None), ("auto", 257, "split"), ("split", 8, "split"), ("member", 256, None),
                                                            ("member", 257, "batch size 257 > 256"), ("auto", 1025, "batch size 1025 > 1024")])
def test_the_kernel_a_batch_size_is_sent_to(step_kernel, batch_size, sent):
    mlp = tr.TinyGaussianMLP(2, 4, 8, 3, 3)
    tr.load_params(mlp, *tr.random_model(2, 4, 8, 3, 3, 0, dtype=torch.float32))
    rng = np.random.default_rng(0)
    obs = rng.standard_normal((1100, 3)).astype(np.float32)
    ds = tr.TransitionIterator(tr.Batch(obs=obs, act=obs[:, :1], next_obs=obs * 1.1), batch_size)
    engine = _Recorder()
    trainer = hipets.ModelTrainer(tr.TinyDynamicsModel(mlp), engine=engine, step_kernel=step_kernel)
    if sent is not None and sent.startswith("batch size"):
        with pytest.raises(hipets.UnsupportedModelError, match=sent):
            trainer.train(ds, num_epochs=1, evaluate=False)
    else:
        trainer.train(ds, num_epochs=1, evaluate=False)
        assert engine.kernels == [sent]  # (None: the keyword is not passed, the engine's default runs)


def test_an_unknown_step_kernel_is_refused():
    with pytest.raises(ValueError, match="step_kernel"):
        hipets.ModelTrainer(tr.TinyDynamicsModel(tr.TinyGaussianMLP(2, 4, 8, 3, 3)), engine=tr.CpuEngine(), step_kernel="rows")
