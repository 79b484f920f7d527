"""Training the DAE on MI355X: the two compiled functions of the reference's
train_dae.py:334-338,

    train_fn(H..., Y_in, T) -> loss          (+ the optimizer's updates)
    val_fn(H..., Y_in, T)   -> [loss, jacc(2, C), mse]

for dae kind 'contextmod'  and kind 'standard' with h at a pool point (section 12).
Forward and data gradient run on the inference layers (ops.Conv), the loss and the optimizer step on
csrc/ctx_train.hip, the weight gradients there (context module) or on csrc/conv_wgrad.hip (standard DAE) --
DAETrainer; and the two of train_fcn8.py:116-137 for the segmentation nets themselves -- _NetTrainer (DESIGN.md
section 24), which FCN8Trainer (section 14) and DenseNetTrainer (section 21) only name and give their defaults.
Everything is enqueued on the current stream; nothing here waits for the device.
"""
import functools

import torch

from . import _lib, ops
from .api import Metrics
from .params import check_mode

SUPPORTED_LOSSES = ('crossentropy', 'squared_error')


# The mode of a run's 16-bit switch (host only): 'f32', or 'bf16' with float32 -- check_x(mode, dtype).
check_wgrad = functools.partial(check_mode, 'wgrad')      # the weight gradients
check_dgrad = functools.partial(check_mode, 'dgrad')      # the data gradients
check_kxk = functools.partial(check_mode, 'kxk')          # FCN-8's fc6 / fc7 gradients
check_fwd = functools.partial(check_mode, 'fwd')          # the training forward, FCN-8's or the standard DAE's
check_deconv = functools.partial(check_mode, 'deconv')    # FC-DenseNet's TransitionUp gradients


def check_supported(kind='contextmod',training_loss=('crossentropy',), ae_h=False, full_im_ft=False,
                    optimizer='rmsprop', dae_dict=None, wgrad='f32', dtype='float32', dgrad='f32', fwd='f32'):
    """Raises NotImplementedError / ValueError with the reason for everything this slice does not train
    (host only: callable before any GPU work).  dae_dict: the standard kind's options (concat_h, bn, dropout,
    conv_before_pool, unpool_type).  wgrad, dgrad, fwd, dtype: the weight-gradient, data-gradient and forward modes
    and the run's precision."""
    if kind not in ('contextmod', 'standard'):
        raise NotImplementedError("training is built for dae kinds 'contextmod' and 'standard' (got %r): the "
                                  'fcn8 kind (strided 4x4 transposed convolutions) has no weight-gradient '
                                  'kernel' % (kind,))
    check_wgrad(wgrad, dtype)
    if wgrad == 'bf16' and kind == 'contextmod':
        raise NotImplementedError("wgrad='bf16' is the zero-padded 3x3 weight gradient of dae kind 'standard' and "
                                  "of FCN-8: the context module's 11-channel gradient kernels stay float32")
    check_dgrad(dgrad, dtype)
    if dgrad == 'bf16' and kind == 'contextmod':
        raise NotImplementedError("dgrad='bf16' is the zero-padded 3x3 data gradient of dae kind 'standard' and "
                                  "of FCN-8: the context module's masked data-gradient kernels stay float32")
    check_fwd(fwd, dtype)
    if fwd == 'bf16' and kind == 'contextmod':
        raise NotImplementedError("fwd='bf16' is the forward of dae kind 'standard' (its 3x3 layers on the 16-bit "
                                  "matrix pipe) and of FCN-8: the context module's dilated 11-channel layers stay "
                                  "float32")
    if kind == 'standard':
        dd = dae_dict or {}
        concat_h = list(dd.get('concat_h', ['input']))
        if not concat_h or 'pool' not in concat_h[-1]:
            raise NotImplementedError("dae kind 'standard' trains with h at a pool point (concat_h ending in "
                                      "'pool*', e.g. ['pool4']); 'contextmod' is the kind that trains with "
                                      "concat_h=['input'] (got concat_h=%r)" % (concat_h,))
        if dd.get('bn', 0):
            raise NotImplementedError("training dae kind 'standard': bn=1 (batch statistics) is not built")
        if float(dd.get('dropout', 0) or 0) > 0:
            raise NotImplementedError("training dae kind 'standard': dropout > 0 is not built")
        if int(dd.get('conv_before_pool', 1)) != 1:
            raise NotImplementedError("training dae kind 'standard': conv_before_pool must be 1")
        if dd.get('unpool_type', 'trackind') not in ('trackind', 'inverse'):
            raise NotImplementedError("training dae kind 'standard': unpool_type must be 'trackind' or 'inverse' "
                                      "(unpool_type='standard', the 4x4 transposed convolution, is not built)")
    for name in training_loss:
        if name not in SUPPORTED_LOSSES:
            raise NotImplementedError('training loss %r is not built (supported: %s)'
                                      % (name, ', '.join(SUPPORTED_LOSSES)))
    if not training_loss:
        raise ValueError('training_loss is empty')
    if ae_h:
        raise NotImplementedError('ae_h (Plug&Play: the DAE on h itself, train_dae.py:177-178) is not built')
    if full_im_ft:
        raise NotImplementedError('full_im_ft (full-image fine-tuning) is not built')
    if optimizer not in ops.OPTIMIZERS:
        raise ValueError('Unknown optimizer')                      # train_dae.py:330-331


class _Trainer:
    """What the trainers share: the optimizer state of a net's flat parameter buffer, the learning rate the
    kernels read, the generator, and val_fn's softmax + confusion counts."""

    def __init__(self, net, n_classes, void_labels, optimizer, learning_rate, seed):
        if list(void_labels) not in ([n_classes], []):
            raise NotImplementedError('void_labels must be [n_classes] (the last target channel) or empty')
        self.C, self.optimizer = int(n_classes), optimizer
        dev, dt = net.flat.device, net.flat.dtype
        self.lr = torch.full((1,), float(learning_rate), dtype=dt, device=dev)     # read by the kernel
        self.s1 = torch.zeros_like(net.flat)
        self.s2 = torch.zeros_like(net.flat) if optimizer == 'adam' else None
        self.state = torch.tensor([0.0, 1.0, 1.0], dtype=dt, device=dev) if optimizer == 'adam' else None
        self.generator = None
        if seed is not None:
            self.generator = torch.Generator(device=dev)
            self.generator.manual_seed(int(seed))

    def set_learning_rate(self, lr):
        self.lr.fill_(float(lr))

    def _metrics(self, score, T):
        """The Metrics of one batch: the softmax of `score`, then its confusion counts against T."""
        pred = ops.crop_softmax(score, score.shape[2], score.shape[3], off=(0, 0))
        m = Metrics(self.C, score.device)
        ops.confusion_accumulate(pred, T, m.cm, m.sums)
        return m


class DAETrainer(_Trainer):
    """fcn: the segmentation net (callable X -> [H..., Y]; may be None when the caller brings H and Y);
    dae: a ContextModDAE, or a StandardDAE built with trainable=True; trained in place."""

    def __init__(self, fcn, dae, n_classes, void_labels=(11,), optimizer='rmsprop', learning_rate=1e-4,
                 training_loss=('crossentropy',), lmb=1.0, noise=0.0, seed=None):
        kind = getattr(dae, 'kind', None)
        if kind == 'standard' and not dae.trainable:
            raise NotImplementedError('training a StandardDAE needs one built with trainable=True')
        check_supported(kind, training_loss, optimizer=optimizer, dae_dict={'concat_h': getattr(dae, 'concat_h', ())})
        self.grid = kind == 'standard'     # millions of parameters: the many-workgroup optimizer step, same bits
        super().__init__(dae, n_classes, void_labels, optimizer, learning_rate, seed)
        self.fcn, self.dae = fcn, dae
        self.losses, self.lmb, self.noise = tuple(training_loss), float(lmb), float(noise)

    def anneal(self, factor):
        """lr <- lr * factor on the device (train_dae.py:424)."""
        self.lr.mul_(float(factor))

    def train_step(self, H, Y_in, T, eps=None):
        """One step of train_fn (H: the h maps, one per concat point, or the only one): returns the loss BEFORE
        the update as a device scalar (float64)."""
        dae = self.dae
        score = dae.forward_train(H if isinstance(H, (list, tuple)) else [H], Y_in, noise=self.noise,
                                  generator=self.generator, eps=eps)
        res, g, _ = ops.ctx_loss(score, T, self.losses, self.lmb, grad=True)
        dae.backward(g)
        ops.opt_step(self.optimizer, dae.flat, dae.gflat, self.s1, self.s2, self.lr, self.state, grid=self.grid)
        dae.refresh()
        return res[0]

    def val_step(self, H, Y_in, T):
        """val_fn (deterministic: no noise): (loss, Metrics, mse) -- loss and mse device scalars, the
        Jaccard counts in the Metrics accumulators (api.Metrics.result() -> acc, jacc(2, C), mse)."""
        dae = self.dae
        score = dae.forward_train(H if isinstance(H, (list, tuple)) else [H], Y_in, noise=0.0)
        res, _, _ = ops.ctx_loss(score, T, self.losses, self.lmb, grad=False)
        return res[0], self._metrics(score, T), res[2]


class _NetTrainer(_Trainer):
    """train_fn / val_fn of a segmentation net built with trainable=True, trained in place: train_fn = masked
    cross-entropy + weight_decay * sum p^2 over the net's weight_ranges(), val_fn = loss and Jaccard counts on the
    deterministic forward.  A subclass names the net (_NET) and says in its constructor which optimizer and
    learning rate it defaults to and whether the optimizer can be chosen."""

    _NET = None

    def __init__(self, net, n_classes, void_labels, optimizer, learning_rate, weight_decay, seed):
        if not getattr(net, 'trainable', False):
            raise NotImplementedError('training %s needs one built with trainable=True' % self._NET)
        if optimizer not in ops.OPTIMIZERS:
            raise ValueError('Unknown optimizer')
        if not float(weight_decay) >= 0.0:
            raise ValueError('weight_decay must be >= 0')
        super().__init__(net, n_classes, void_labels, optimizer, learning_rate, seed)
        self.net, self.weight_decay = net, float(weight_decay)
        self.ranges = self.chunks(net.weight_ranges())     # a list of CHUNKS of ranges: one ops.l2_term call each

    @staticmethod
    def chunks(ranges, step=_lib.L2_MAX_RANGES):
        """ops.l2_term takes a bounded number of ranges per launch (FC-DenseNet has two hundred, FCN-8 twenty-one)."""
        return [ranges[i:i + step] for i in range(0, len(ranges), step)]

    def anneal(self, factor):
        """lr <- lr * factor on the device."""
        self.lr.mul_(float(factor))

    def train_step(self, X, T, *masks, **mask_kw):
        """One step of train_fn: returns the loss BEFORE the update as a device scalar (float64).  masks: the
        caller's dropout masks as net.forward_train takes them (tests), else drawn from the trainer's generator.
        No host wait."""
        net = self.net
        score = net.forward_train(X, *masks, generator=self.generator, **mask_kw)
        res, g, _ = ops.ctx_loss(score, T, ('crossentropy',), 1.0, grad=True)
        net.backward(g)
        loss = res[0]
        if self.weight_decay > 0:
            for chunk in self.ranges:
                loss = loss + self.weight_decay * ops.l2_term(net.flat, net.gflat, chunk, self.weight_decay)[0]
        ops.opt_step(self.optimizer, net.flat, net.gflat, self.s1, self.s2, self.lr, self.state, grid=True)
        net.refresh()
        return loss

    def val_step(self, X, T):
        """val_fn (deterministic: no dropout): (loss, Metrics) -- the loss a device scalar, accuracy and the
        Jaccard counts in the Metrics accumulators (api.Metrics.result() -> acc, jacc(2, C), mse)."""
        score = self.net.forward_train(X, deterministic=True)
        res, _, _ = ops.ctx_loss(score, T, ('crossentropy',), 1.0, grad=False)
        return res[0], self._metrics(score, T)


class FCN8Trainer(_NetTrainer):
    """The two compiled functions of the reference's train_fcn8.py:116-137 for an FCN8, under
    adam; train_step(X, T, keep6, keep7)."""

    _NET = 'an FCN8'

    def __init__(self, net, n_classes, void_labels=(11,), learning_rate=1e-4, weight_decay=0.0, seed=None):
        super().__init__(net, n_classes, void_labels, 'adam', learning_rate, weight_decay, seed)


class DenseNetTrainer(_NetTrainer):
    """For an FCDenseNet (the reference has no FC-DenseNet training script: optimizer and
    schedule are restated from upstream FC-DenseNet), under RMSprop (default) or adam; the weight decay is over every
    W and every gamma (lasagne marks gamma regularizable; never beta or a bias); train_step(X, T, keeps), one mask
    per 'brc' / 'td' layer.  The 16-bit modes (wgrad, deconv, fwd) are the net's own: train_fn and val_fn run whatever
    its forward_train and backward run."""

    _NET = 'an FCDenseNet'

    def __init__(self, net, n_classes, void_labels=(11,), optimizer='rmsprop', learning_rate=1e-3, weight_decay=0.0,
                 seed=None):
        super().__init__(net, n_classes, void_labels, optimizer, learning_rate, weight_decay, seed)
