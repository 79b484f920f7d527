#!/usr/bin/env python3
"""Training FCN-8 on MI355X -- counterpart of the reference's train_fcn8.py, the first stage of its workflow: it
writes the `fcn8_model.npz`-format checkpoint every other entry point loads (buildFCN8(path_weights=...)).

Same arguments and defaults (`-dataset`, `-learning_rate`, `-penal_cst`, `--num_epochs` / `-ne`, `-max_patience`,
`-batch_size`, `-data_augmentation`, `-early_stop_class`, `-train_from_0_255`; train_fcn8.py:274-317; the list /
dict arguments are JSON), the same epoch loop (train_fcn8.py:150-271: adam on the masked cross-entropy +
penal_cst * sum W^2, a validation pass, the mean validation Jaccard or the `early_stop_class` one, the best / last
/ patience rule with its `epoch > 1` condition, the final test pass on the best weights, copy_tree to loadpath) and
the same files in savepath/<dataset>/<exp_name>/: `new_fcn8_model_best.npz` / `new_fcn8_model_last.npz` (np.savez
of W, b per layer in fcn8.PARAM_ORDER), `fcn8_errors_best.npz` / `fcn8_errors_last.npz`, `fcn8_output.log`,
`config.txt`.  The lab paths keyed on getuser() become `--savepath / --loadpath`; `--synthetic` supplies the seeded
synthetic split; `--width_div / --fc_channels` shrink the net (tests).

Two quirks of the reference, the first kept, the second fixed:
  * `exp_name = 'fcn8_' + 'data_aug' if bool(data_augmentation) else ''` parses as `('fcn8_' + 'data_aug') if ...
    else ''`: the folder is `fcn8_data_aug` with augmentation and the dataset folder itself without.  Kept.
  * `os.path.join(savepath + "fcn8_errors_best.npz")` lacks the separator and writes NEXT TO the folder.  Here the
    error files are written inside it.
Initial weights without `--resume`: GlorotUniform W and zero b, Lasagne's default when load_weights=False, seeded
and drawn on the host.  The reference starts from PASCAL-VOC .mat weights (pascal=True); that import is not built
and `-pascal` is refused as buildFCN8 refuses it.  Data augmentation is recorded (it names the folder and sets the
synthetic crop) but not applied.  What is refused exits with status 2 and the reason on stderr before any GPU
work.  All arithmetic runs in the HIP kernels of libiiseg_hip.so.
`--wgrad bf16` (float32 only) forms the weight gradients of the thirteen 3x3 layers on the
16-bit matrix pipe from operands rounded once to bf16; fc6, fc7, the score and transposed layers, the forward, the
data gradients, the parameters, adam's state and the checkpoints stay float32, so the experiment folder keeps its
name (config.txt records the mode).  With `--dtype float64` it is refused like the rest.
`--dgrad bf16` (the same conditions) forms the twelve 3x3 data gradients of the backward pass on
the 16-bit matrix pipe from the parameters and g_z rounded once to bf16; config.txt records it as well.
`--kxk bf16` (the same conditions) forms the weight and data gradients of fc6 and fc7 on the
16-bit matrix pipe, likewise; config.txt records it as well.
`--fwd bf16` (the same conditions) runs the thirteen 3x3 layers, fc6 and fc7 of the training and
validation forward on the 16-bit matrix pipe, operands rounded once to bf16, fp32 accumulation and fp32 maps;
config.txt records it as well.
"""
import os
import sys

import numpy as np

from iterative_inference_segm_amd import train_loop
from iterative_inference_segm_amd.train_loop import one_hot_void_last      # noqa: F401  (the drivers' own name for it)

DATA_AUGMENTATION = {'crop_size': [224, 224], 'horizontal_flip': True, 'fill_mode': 'constant'}   # :301
SWITCHES = {'wgrad': 'the thirteen 3x3 layers', 'dgrad': 'the twelve 3x3 layers of the backward pass',
            'kxk': 'weights and data', 'fwd': 'the 3x3 layers, fc6 and fc7, in training and validation'}


def _bool(s):
    return str(s).lower() in ('1', 'true', 'yes')


def experiment_name(data_augmentation):
    """train_fcn8.py:53, with its operator precedence."""
    return 'fcn8_' + 'data_aug' if bool(data_augmentation) else ''


def glorot_params(shapes, seed):
    """{name: (W, b)}: lasagne.init.GlorotUniform (gain 1) W -- limit sqrt(6 / ((n0 + n1) k k)) for W[n0,n1,k,k],
    which is what both Conv2DLayer and Deconv2DLayer get -- and zero b, seeded, in the order of `shapes`."""
    rng = np.random.default_rng(seed)
    out = {}
    for name, (wshape, nb) in shapes.items():
        a = np.sqrt(6.0 / ((wshape[0] + wshape[1]) * wshape[2] * wshape[3]))
        out[name] = (rng.uniform(-a, a, size=wshape).astype(np.float32), np.zeros(nb, np.float32))
    return out


def check_supported(dataset, savepath, pascal=False, dtype='float32', batch_size=(10, 1, 1), num_epochs=1,
                    max_patience=1, learning_rate=1e-4, weight_decay=0.0, early_stop_class=None, wgrad='f32',
                    dgrad='f32', kxk='f32', fwd='f32'):
    """Everything this build does not train and every bad argument, refused with the reason (host only)."""
    train_loop.check_savepath(savepath)
    if pascal:
        raise NotImplementedError('pascal .mat weights are not supported')              # as buildFCN8
    train_loop.check_dataset(dataset)
    if dtype not in ('float32', 'float64'):
        raise NotImplementedError('training FCN-8: float32 or float64; the 16-bit legs are not trained')
    train_loop.check_switches(dtype, wgrad=wgrad, dgrad=dgrad, kxk=kxk, fwd=fwd)
    train_loop.check_schedule(batch_size, num_epochs, max_patience)
    if not float(learning_rate) > 0 or not float(weight_decay) >= 0:
        raise ValueError('learning_rate must be > 0 and penal_cst >= 0')
    if early_stop_class is not None and int(early_stop_class) < 0:
        raise ValueError('early_stop_class must be a class index')


def train(dataset, learn_step=0.005, weight_decay=1e-4, num_epochs=500, max_patience=100, data_augmentation={},
          savepath=None, loadpath=None, early_stop_class=None, batch_size=None, resume=False,
          train_from_0_255=False, synthetic=False, n_images=20, image_size=None, seed=0, dtype='float32',
          width_div=1, fc_channels=4096, max_batches=None, wgrad='f32', dgrad='f32', kxk='f32', fwd='f32',
          verbose=True):
    """Signature of reference train_fcn8.py:41-48 plus keyword-only extras.  wgrad ('f32' | 'bf16': the 3x3 weight
    gradients' operand precision) is recorded in config.txt and stays out of the experiment name: the checkpoints
    are float32 either way; dgrad (the 3x3 data gradients'), kxk (fc6's and fc7's gradients) and fwd (the training
    forward's fifteen wide layers) likewise.  Returns the per-epoch lists and the experiment folder."""
    bs = list(batch_size) if batch_size is not None else [10, 1, 1]                     # :84-87
    check_supported(dataset, savepath, False, dtype, bs, num_epochs, max_patience, learn_step, weight_decay,
                    early_stop_class, wgrad, dgrad, kxk, fwd)
    say = print if verbose else (lambda *a, **k: None)
    savepath, loadpath = train_loop.experiment_folders(
        savepath, loadpath, dataset, experiment_name(data_augmentation),
        dict(dataset=dataset, learn_step=learn_step, weight_decay=weight_decay, num_epochs=num_epochs,
             max_patience=max_patience, data_augmentation=data_augmentation, early_stop_class=early_stop_class,
             batch_size=bs, resume=resume, train_from_0_255=train_from_0_255, seed=seed, dtype=dtype,
             width_div=width_div, fc_channels=fc_channels, wgrad=wgrad, dgrad=dgrad, kxk=kxk, fwd=fwd), say)

    # ---- from here on: the GPU ----
    import torch
    from iterative_inference_segm_amd import synthetic as S
    from iterative_inference_segm_amd.data_loader import load_data
    from iterative_inference_segm_amd.fcn8 import FCN8, PARAM_ORDER
    from iterative_inference_segm_amd.train import FCN8Trainer
    from iterative_inference_segm_amd.weights import load_param_list, save_param_list

    tdt = {'float32': torch.float32, 'float64': torch.float64}[dtype]
    crop = (data_augmentation or {}).get('crop_size')
    size = tuple(image_size) if image_size is not None else (tuple(crop) if crop else (360, 480))
    train_iter, val_iter, test_iter = load_data(dataset, data_augmentation, one_hot=False, batch_size=bs,
                                                return_0_255=train_from_0_255,
                                                synthetic=True if synthetic else None, n_images=n_images,
                                                image_size=size)
    n_classes, void_labels = train_iter.non_void_nclasses, train_iter.void_labels
    nb_in_channels = train_iter.data_shape[0]
    if early_stop_class is not None and int(early_stop_class) >= n_classes:
        raise ValueError('early_stop_class must be below %d' % n_classes)
    nb = lambda it: it.nbatches if max_batches is None else min(it.nbatches, int(max_batches))
    say('Batch. train: %d, val %d, test %d' % (nb(train_iter), nb(val_iter), nb(test_iter) if test_iter else 0))
    say('Nb of classes: %d' % n_classes)
    say('Nb. of input channels: %d' % nb_in_channels)

    best_path = os.path.join(savepath, 'new_fcn8_model_best.npz')
    if resume:
        params = load_param_list(os.path.join(loadpath, 'new_fcn8_model_best.npz'), PARAM_ORDER)
    else:
        like = S.make_fcn8_params(nb_in_channels, n_classes, seed=1234, width_div=width_div, fc_channels=fc_channels)
        params = glorot_params({n: (like[n][0].shape, like[n][1].shape[0]) for n in PARAM_ORDER}, 4321 + int(seed))
    net = FCN8(params, n_classes, layer=['probs_dimshuffle'], dtype=tdt, mma='f32', trainable=True,
               wgrad=wgrad, dgrad=dgrad, kxk=kxk, fwd=fwd)
    trainer = FCN8Trainer(net, n_classes, void_labels, learning_rate=learn_step, weight_decay=weight_decay, seed=seed)

    def save(tag, errors):
        save_param_list(os.path.join(savepath, 'new_fcn8_model_%s.npz' % tag), net.state_arrays(), PARAM_ORDER)
        np.savez(os.path.join(savepath, 'fcn8_errors_%s.npz' % tag), *[np.asarray(e) for e in errors])

    def reload_best():
        """The best weights back into the net's own buffer, in place; False: this run wrote none."""
        if not os.path.exists(best_path):
            return False
        for name, (W, b) in load_param_list(best_path, PARAM_ORDER).items():
            Wd, bd = net.parameters()[name]
            Wd.copy_(torch.from_numpy(W).to(tdt))
            bd.copy_(torch.from_numpy(b).to(tdt))
        net.refresh()
        return True

    mean_jaccard = lambda jacc_tot: float(np.mean(train_loop.per_class_jaccard(jacc_tot)))
    class_jaccard = lambda jacc_tot: float(train_loop.per_class_jaccard(jacc_tot)[int(early_stop_class)])
    say('Start training')
    lists = train_loop.run_epochs(
        num_epochs, max_patience, rule=train_loop.fcn8_rule,                            # :208-224, `epoch > 1` kept
        train_pass=lambda: train_loop.train_steps(trainer, train_iter, nb(train_iter), n_classes),
        n_train=nb(train_iter), val_pass=lambda: train_loop.evaluate(trainer, val_iter, nb(val_iter), n_classes),
        metric=mean_jaccard if early_stop_class is None else class_jaccard, save=save,  # :189-192
        log_path=os.path.join(savepath, 'fcn8_output.log'),
        test_pass=None if test_iter is None else
        lambda: train_loop.evaluate(trainer, test_iter, nb(test_iter), n_classes),
        test_metric=mean_jaccard, reload_best=reload_best, best_name='new_fcn8_model_best.npz',
        savepath=savepath, loadpath=loadpath, say=say)
    return dict(zip(('err_train', 'err_valid', 'acc_valid', 'jacc_valid'), lists), savepath=savepath,
                loadpath=loadpath)


def make_parser():
    parser = train_loop.make_parser('FCN-8 training', SWITCHES)
    parser.add_argument('-learning_rate', default=0.0001, help='Learning Rate')
    parser.add_argument('-penal_cst', default=0.0, help='regularization constant')
    parser.add_argument('-max_patience', type=int, default=100, help='Max patience')
    parser.add_argument('-batch_size', type=train_loop.json_arg, default=[10, 1, 1],
                        help='Batch size [train, val, test] (JSON)')
    parser.add_argument('-data_augmentation', type=train_loop.json_arg, default=dict(DATA_AUGMENTATION),
                        help='use data augmentation (JSON): recorded, names the experiment folder; crop_size sets '
                             'the synthetic image size')
    parser.add_argument('-early_stop_class', type=int, default=None, help='class to early stop on')
    parser.add_argument('-train_from_0_255', type=_bool, default=False,
                        help='Whether to train from images within 0-255 range')
    parser.add_argument('-pascal', type=_bool, default=False, help='start from PASCAL .mat weights (refused)')
    parser.add_argument('--width_div', type=int, default=1, help='divide the channel counts (small nets for tests)')
    parser.add_argument('--fc_channels', type=int, default=4096)
    return parser


def parse_args(argv=None):
    return make_parser().parse_args(argv)


def main(argv=None):
    a = parse_args(argv)
    return train_loop.main(
        'train_fcn8.py',
        lambda: check_supported(a.dataset, a.savepath, a.pascal, a.dtype, a.batch_size, a.num_epochs, a.max_patience,
                                a.learning_rate, a.penal_cst, a.early_stop_class, a.wgrad, a.dgrad, a.kxk, a.fwd),
        lambda: train(a.dataset, float(a.learning_rate), float(a.penal_cst), int(a.num_epochs), int(a.max_patience),
                      data_augmentation=a.data_augmentation, batch_size=a.batch_size,
                      early_stop_class=a.early_stop_class, savepath=a.savepath, loadpath=a.loadpath, resume=a.resume,
                      train_from_0_255=a.train_from_0_255, synthetic=a.synthetic, n_images=a.n_images,
                      image_size=a.image_size, seed=a.seed, dtype=a.dtype, width_div=a.width_div,
                      fc_channels=a.fc_channels, max_batches=a.max_batches, wgrad=a.wgrad, dgrad=a.dgrad, kxk=a.kxk,
                      fwd=a.fwd))


if __name__ == '__main__':
    sys.exit(main())
