"""Training the context-module DAE on MI355X: the two compiled functions of the reference's
train_dae.py:334-338,

    train_fn(H..., Y_in, T) -> loss          (+ the optimizer's updates)
    val_fn(H..., Y_in, T)   -> [loss, jacc(2, C), mse]

for dae kind 'contextmod' (DESIGN.md section 9).  Forward and data gradient run on the inference layers
(ops.Conv), the loss, the weight gradients and the optimizer step on csrc/ctx_train.hip.  Everything is
enqueued on the current stream; nothing here waits for the device.
"""
import torch

from . import ops
from .api import Metrics
from .contextmod import ContextModDAE

SUPPORTED_LOSSES = ('crossentropy', 'squared_error')


def check_supported(kind='contextmod', training_loss=('crossentropy',), ae_h=False, full_im_ft=False,
                    optimizer='rmsprop'):
    """Raises NotImplementedError / ValueError with the reason for everything this slice does not train
    (host only: callable before any GPU work)."""
    if kind != 'contextmod':
        raise NotImplementedError("training is built for dae kind 'contextmod' only (got %r): the standard "
                                  'and fcn8 kinds need weight gradients at 64-2048 channels' % (kind,))
    for name in training_loss:
        if name not in SUPPORTED_LOSSES:
            raise NotImplementedError('training loss %r is not built (supported: %s)'
                                      % (name, ', '.join(SUPPORTED_LOSSES)))
    if not training_loss:
        raise ValueError('training_loss is empty')
    if ae_h:
        raise NotImplementedError("ae_h (Plug&Play) needs dae kind 'standard' (train_dae.py:177-178)")
    if full_im_ft:
        raise NotImplementedError('full_im_ft (full-image fine-tuning) is not built')
    if optimizer not in ops.OPTIMIZERS:
        raise ValueError('Unknown optimizer')                      # train_dae.py:330-331


class DAETrainer:
    """fcn: the segmentation net (callable X -> [H..., Y]; may be None when the caller brings H and Y);
    dae: a ContextModDAE, trained in place."""

    def __init__(self, fcn, dae, n_classes, void_labels=(11,), optimizer='rmsprop', learning_rate=1e-4,
                 training_loss=('crossentropy',), lmb=1.0, noise=0.0, seed=None):
        if not isinstance(dae, ContextModDAE):
            raise NotImplementedError("training is built for dae kind 'contextmod' only")
        check_supported('contextmod', training_loss, optimizer=optimizer)
        if list(void_labels) not in ([n_classes], []):
            raise NotImplementedError('void_labels must be [n_classes] (the last target channel) or empty')
        self.fcn, self.dae, self.C = fcn, dae, int(n_classes)
        self.optimizer, self.losses, self.lmb, self.noise = optimizer, tuple(training_loss), float(lmb), float(noise)
        dev, dt = dae.flat.device, dae.flat.dtype
        self.lr = torch.full((1,), float(learning_rate), dtype=dt, device=dev)     # read by the kernel
        self.s1 = torch.zeros_like(dae.flat)
        self.s2 = torch.zeros_like(dae.flat) if optimizer == 'adam' else None
        self.state = torch.tensor([0.0, 1.0, 1.0], dtype=dt, device=dev) if optimizer == 'adam' else None
        self.generator = None
        if seed is not None:
            self.generator = torch.Generator(device=dev)
            self.generator.manual_seed(int(seed))

    def set_learning_rate(self, lr):
        self.lr.fill_(float(lr))

    def anneal(self, factor):
        """lr <- lr * factor on the device (train_dae.py:424)."""
        self.lr.mul_(float(factor))

    def _h(self, H):
        if isinstance(H, (list, tuple)):
            if len(H) != 1:
                raise ValueError('expected 1 h tensor, got %d' % len(H))
            return H[0]
        return H

    def train_step(self, H, Y_in, T, eps=None):
        """One step of train_fn: returns the loss BEFORE the update as a device scalar (float64)."""
        dae = self.dae
        score = dae.forward_train(self._h(H), Y_in, noise=self.noise, generator=self.generator, eps=eps)
        res, g, _ = ops.ctx_loss(score, T, self.losses, self.lmb, grad=True)
        dae.backward(g)
        ops.opt_step(self.optimizer, dae.flat, dae._gflat, self.s1, self.s2, self.lr, self.state)
        dae.refresh()
        return res[0]

    def val_step(self, H, Y_in, T):
        """val_fn (deterministic: no noise): (loss, Metrics, mse) -- loss and mse device scalars, the
        Jaccard counts in the Metrics accumulators (api.Metrics.result() -> acc, jacc(2, C), mse)."""
        dae = self.dae
        score = dae.forward_train(self._h(H), Y_in, noise=0.0)
        res, _, _ = ops.ctx_loss(score, T, self.losses, self.lmb, grad=False)
        pred = ops.crop_softmax(score, score.shape[2], score.shape[3], off=(0, 0))
        m = Metrics(self.C, score.device)
        ops.confusion_accumulate(pred, T, m.cm, m.sums)
        return res[0], m, res[2]
