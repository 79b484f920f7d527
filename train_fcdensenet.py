#!/usr/bin/env python3
"""Training FC-DenseNet on MI355X: writes the `FC-DenseNet103_weights.npz`-format checkpoint that
build_fcdensenet(weight_path=...), train_dae.py and iterative_inference.py load.

The reference has no FC-DenseNet training script; it loads weights trained with upstream FC-DenseNet (SimJeg).  What
this driver takes from upstream is restated from memory and cannot be verified here: Dropout(0.2) behind the
convolution of every BN_ReLU_Conv and TransitionDown, RMSprop with learning rate 1e-3 decayed by 0.995 per epoch,
weight decay 1e-4 on every regularizable parameter (every W and every BatchNorm gamma), batch 3 on 224 x 224 crops.
The epoch loop, the early stopping on the mean validation Jaccard (patience rule) and the file layout follow
train_fcn8.py -- except that the best checkpoint is also written after the first epoch, so that a run of any length
leaves one.  In savepath/<dataset>/fc_densenet/: `FC-DenseNet103_weights_best.npz` / `_last.npz` (np.savez in
get_all_param_values order: per BatchNorm beta, gamma, mean, inv_std -- the running averages, alpha 0.1 -- then W, b
per convolution), `errors_best.npz` / `errors_last.npz`, `output.log`, `config.txt`.  Copied to
<weights_path>/<dataset>/FC-DenseNet103_weights.npz, the best checkpoint is what the other entry points load.
Initial weights without `--resume`: HeUniform W, zero b, gamma 1, beta 0 (upstream's), seeded and drawn on the host.
`--layers_per_block / --growth / --n_first` shrink the net (tests); such a checkpoint records its architecture.
`--wgrad bf16` (float32 only) forms the weight gradients of the zero-padded 3x3 layers on the
16-bit matrix pipe, in blocks of 16 output channels for the dense-block layers; everything else stays float32, and
the experiment folder and the checkpoint names do not change (config.txt records the mode).
`--deconv bf16` (float32 only) does the same for the data and weight gradients of the five
TransitionUp layers (K = 3, stride-2 transposed convolutions); config.txt records it, no name changes.
`--fwd bf16` (float32 only) runs every dense-block layer's BatchNorm + ReLU + 3x3 convolution +
dropout as one launch on the 16-bit matrix pipe, in training and in validation; config.txt records it, no name changes.
Data augmentation is not built.  What is refused exits with status 2 and the reason on stderr before any GPU work.
All arithmetic runs in the HIP kernels of libiiseg_hip.so.
"""
import os
import sys

import numpy as np

from iterative_inference_segm_amd import train_loop
from iterative_inference_segm_amd.train_loop import one_hot_void_last      # noqa: F401  (the drivers' own name for it)

EXP_NAME = 'fc_densenet'
MODEL = 'FC-DenseNet103_weights_%s.npz'
LAYERS_PER_BLOCK = [4, 5, 7, 10, 12, 15, 12, 10, 7, 5, 4]
OPTIMIZERS = ('rmsprop', 'adam')
MMA_MODES = ('f32', 'bf16', 'bf16c8', 'bf16x3')
SWITCHES = {'wgrad': 'the zero-padded 3x3 layers', 'deconv': 'the five TransitionUp layers, weights and data',
            'fwd': 'the dense-block 3x3 layers, in training and validation'}


def check_supported(dataset, savepath, dtype='float32', mma='f32', optimizer='rmsprop', dropout=0.2,
                    batch_size=(3, 1, 1), num_epochs=1, max_patience=1, learning_rate=1e-3, lr_decay=0.995,
                    weight_decay=1e-4, layers_per_block=LAYERS_PER_BLOCK, growth=16, n_first=48, image_size=None,
                    wgrad='f32', deconv='f32', fwd='f32'):
    """Everything this build does not train and every bad argument, refused with the reason (host only)."""
    train_loop.check_savepath(savepath)
    train_loop.check_dataset(dataset)
    if mma not in MMA_MODES:
        raise ValueError('mma must be one of %s' % ', '.join(MMA_MODES))
    if dtype not in ('float32', 'float64') or (dtype == 'float32' and mma != 'f32'):
        raise NotImplementedError("training FC-DenseNet: float32 (mma 'f32') or float64; the 16-bit legs (dtype %s, "
                                  'mma %r) are not trained' % (dtype, mma))
    train_loop.check_switches(dtype, wgrad=wgrad, deconv=deconv, fwd=fwd)
    if optimizer not in OPTIMIZERS:
        raise ValueError('Unknown optimizer')
    if not 0.0 <= float(dropout) < 1.0:
        raise ValueError('dropout must be in [0, 1)')
    train_loop.check_schedule(batch_size, num_epochs, max_patience)
    if not float(learning_rate) > 0 or not float(weight_decay) >= 0 or not 0 < float(lr_decay) <= 1:
        raise ValueError('learning_rate must be > 0, weight_decay >= 0 and lr_decay in (0, 1]')
    lpb = list(layers_per_block)
    if len(lpb) < 3 or len(lpb) % 2 != 1 or any(int(v) < 1 for v in lpb) or int(growth) < 1 or int(n_first) < 1:
        raise ValueError('layers_per_block: an odd number (2 n_pool + 1) of positive counts; growth, n_first >= 1')
    if image_size is not None:
        n_pool = len(lpb) // 2
        if any(int(v) >> n_pool < 1 for v in image_size):
            raise ValueError('image_size %s is too small for %d pools' % (list(image_size), n_pool))


def he_params(plan, seed):
    """Creation-order parameter dicts for `plan` (densenet.layer_plan): HeUniform W (limit sqrt(6 / fan_in)), zero
    b, gamma 1, beta 0; seeded."""
    rng = np.random.default_rng(seed)
    out = []
    for kind, cin, cout in plan:
        p = {'kind': kind}
        if kind in ('brc', 'td'):
            p['gamma'], p['beta'] = np.ones(cin, np.float32), np.zeros(cin, np.float32)
        k = 1 if kind in ('td', 'softmax') else 3
        shape, fan = ((cin, cout, 3, 3), cout * 9) if kind == 'tu' else ((cout, cin, k, k), cin * k * k)
        a = np.sqrt(6.0 / fan)
        p['W'] = rng.uniform(-a, a, size=shape).astype(np.float32)
        p['b'] = np.zeros(cout, np.float32)
        out.append(p)
    return out


def train(dataset, learning_rate=1e-3, lr_decay=0.995, weight_decay=1e-4, num_epochs=750, max_patience=150,
          savepath=None, loadpath=None, batch_size=None, resume=False, synthetic=False, n_images=20, image_size=None,
          seed=0, dtype='float32', mma='f32', optimizer='rmsprop', dropout=0.2, layers_per_block=LAYERS_PER_BLOCK,
          growth=16, n_first=48, max_batches=None, verbose=True, wgrad='f32', deconv='f32', fwd='f32'):
    """Returns the per-epoch lists and the experiment folder.  wgrad, deconv, fwd ('f32' | 'bf16'): the operand
    precision of the zero-padded 3x3 weight gradients, of the TransitionUp gradients and of the dense-block layers'
    forward (FCDenseNet's keywords)."""
    bs = list(batch_size) if batch_size is not None else [3, 1, 1]
    lpb = [int(v) for v in layers_per_block]
    size = tuple(image_size) if image_size is not None else (224, 224)
    check_supported(dataset, savepath, dtype, mma, optimizer, dropout, bs, num_epochs, max_patience, learning_rate,
                    lr_decay, weight_decay, lpb, growth, n_first, size, wgrad, deconv, fwd)
    say = print if verbose else (lambda *a, **k: None)
    savepath, loadpath = train_loop.experiment_folders(
        savepath, loadpath, dataset, EXP_NAME,
        dict(dataset=dataset, learning_rate=learning_rate, lr_decay=lr_decay, weight_decay=weight_decay,
             num_epochs=num_epochs, max_patience=max_patience, batch_size=bs, resume=resume, seed=seed, dtype=dtype,
             optimizer=optimizer, dropout=dropout, layers_per_block=lpb, growth=growth, n_first=n_first,
             image_size=list(size), wgrad=wgrad, deconv=deconv, fwd=fwd), say)

    # ---- from here on: the GPU ----
    import torch
    from iterative_inference_segm_amd.data_loader import load_data
    from iterative_inference_segm_amd.densenet import FCDenseNet, layer_plan, load_params, save_checkpoint
    from iterative_inference_segm_amd.train import DenseNetTrainer

    tdt = {'float32': torch.float32, 'float64': torch.float64}[dtype]
    train_iter, val_iter, test_iter = load_data(dataset, {}, one_hot=False, batch_size=bs,
                                                synthetic=True if synthetic else None, n_images=n_images,
                                                image_size=size)
    n_classes, void_labels = train_iter.non_void_nclasses, train_iter.void_labels
    nb_in_channels = train_iter.data_shape[0]
    nb = lambda it: it.nbatches if max_batches is None else min(it.nbatches, int(max_batches))
    say('Batch. train: %d, val %d, test %d' % (nb(train_iter), nb(val_iter), nb(test_iter) if test_iter else 0))
    say('Nb of classes: %d' % n_classes)

    n_pool = len(lpb) // 2
    plan = layer_plan(lpb, n_pool, growth, n_first, nb_in_channels, n_classes)
    best_path = os.path.join(savepath, MODEL % 'best')
    if resume:
        params = load_params(os.path.join(loadpath, MODEL % 'best'), plan)
    else:
        params = he_params(plan, 4321 + int(seed))
    net = FCDenseNet(params, n_classes, layer=[], n_layers_per_block=lpb, n_pool=n_pool, growth=growth, dtype=tdt,
                     mma='f32', trainable=True, dropout=dropout, wgrad=wgrad, deconv=deconv, fwd=fwd)
    trainer = DenseNetTrainer(net, n_classes, void_labels, optimizer=optimizer, learning_rate=learning_rate,
                              weight_decay=weight_decay, seed=seed)

    def save(tag, errors):
        save_checkpoint(os.path.join(savepath, MODEL % tag), net, n_first)
        np.savez(os.path.join(savepath, 'errors_%s.npz' % tag), *[np.asarray(e) for e in errors])

    def reload_best():
        """The best weights back into the net's own buffer, in place (every run has written them)."""
        for p, e in zip(load_params(best_path, plan), net.layers):
            if p['kind'] in ('brc', 'td'):
                e['beta'].copy_(torch.from_numpy(p['beta']).to(tdt))
                e['gamma'].copy_(torch.from_numpy(p['gamma']).to(tdt))
            e['conv'].W.copy_(torch.from_numpy(p['W']).to(tdt))
            e['conv'].b.copy_(torch.from_numpy(p['b']).to(tdt))
        net.refresh()
        return True

    nanmean_jaccard = lambda jacc_tot: float(np.nanmean(train_loop.per_class_jaccard(jacc_tot)))
    say('Start training')
    lists = train_loop.run_epochs(
        num_epochs, max_patience, rule=train_loop.first_epoch_best_rule,
        train_pass=lambda: train_loop.train_steps(trainer, train_iter, nb(train_iter), n_classes),
        n_train=nb(train_iter), val_pass=lambda: train_loop.evaluate(trainer, val_iter, nb(val_iter), n_classes),
        metric=nanmean_jaccard, save=save, log_path=os.path.join(savepath, 'output.log'),
        after_train=lambda: trainer.anneal(lr_decay),
        test_pass=None if test_iter is None else
        lambda: train_loop.evaluate(trainer, test_iter, nb(test_iter), n_classes),
        reload_best=reload_best, best_name=MODEL % 'best', savepath=savepath, loadpath=loadpath, say=say)
    return dict(zip(('err_train', 'err_valid', 'acc_valid', 'jacc_valid'), lists), savepath=savepath,
                loadpath=loadpath)


def make_parser():
    parser = train_loop.make_parser('FC-DenseNet training', SWITCHES)
    parser.add_argument('--learning_rate', type=float, default=1e-3)
    parser.add_argument('--lr_decay', type=float, default=0.995, help='learning-rate factor per epoch')
    parser.add_argument('--weight_decay', type=float, default=1e-4, help='on every W and every gamma')
    parser.add_argument('--batch_size', type=train_loop.json_arg, default=[3, 1, 1], help='[train, val, test] (JSON)')
    parser.add_argument('--max_patience', type=int, default=150)
    parser.add_argument('--mma', default='f32', help="float32: only 'f32' is trained")
    parser.add_argument('--optimizer', default='rmsprop', help='rmsprop | adam')
    parser.add_argument('--dropout', type=float, default=0.2)
    parser.add_argument('--layers_per_block', type=train_loop.json_arg, default=list(LAYERS_PER_BLOCK),
                        help='2 n_pool + 1 layer counts (JSON)')
    parser.add_argument('--growth', type=int, default=16)
    parser.add_argument('--n_first', type=int, default=48)
    return parser


def parse_args(argv=None):
    return make_parser().parse_args(argv)


def main(argv=None):
    a = parse_args(argv)
    return train_loop.main(
        'train_fcdensenet.py',
        lambda: check_supported(a.dataset, a.savepath, a.dtype, a.mma, a.optimizer, a.dropout, a.batch_size,
                                a.num_epochs, a.max_patience, a.learning_rate, a.lr_decay, a.weight_decay,
                                a.layers_per_block, a.growth, a.n_first, a.image_size, a.wgrad, a.deconv, a.fwd),
        lambda: train(a.dataset, a.learning_rate, a.lr_decay, a.weight_decay, a.num_epochs, a.max_patience,
                      savepath=a.savepath, loadpath=a.loadpath, batch_size=a.batch_size, resume=a.resume,
                      synthetic=a.synthetic, n_images=a.n_images, image_size=a.image_size, seed=a.seed, dtype=a.dtype,
                      mma=a.mma, optimizer=a.optimizer, dropout=a.dropout, layers_per_block=a.layers_per_block,
                      growth=a.growth, n_first=a.n_first, max_batches=a.max_batches, wgrad=a.wgrad, deconv=a.deconv,
                      fwd=a.fwd))


if __name__ == '__main__':
    sys.exit(main())
