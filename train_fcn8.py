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
import argparse
import json
import os
import shutil
import sys
import time

import numpy as np

SAVEPATH = os.environ.get('IISEG_SAVEPATH')
LOADPATH = os.environ.get('IISEG_LOADPATH')

DATA_AUGMENTATION = {'crop_size': [224, 224], 'horizontal_flip': True, 'fill_mode': 'constant'}   # :301


def _json(s):
    return json.loads(s) if isinstance(s, str) else s


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


def one_hot_void_last(L, n_classes):
    """Integer labels (B,H,W), void = any label >= n_classes, -> one-hot (B,n_classes+1,H,W), void channel last."""
    L = np.minimum(np.asarray(L).astype(np.int64), n_classes)
    return np.ascontiguousarray(np.moveaxis(np.eye(n_classes + 1, dtype=np.float32)[L], -1, 1))


def check_supported(dataset, savepath, pascal=False, dtype='float32', batch_size=(10, 1, 1), num_epochs=1,
                    max_patience=1, learning_rate=1e-4, weight_decay=0.0, early_stop_class=None, wgrad='f32',
                    dgrad='f32', kxk='f32', fwd='f32'):
    """Everything this build does not train and every bad argument, refused with the reason (host only)."""
    from iterative_inference_segm_amd.train import check_dgrad, check_fwd, check_kxk, check_wgrad
    if savepath is None:
        raise ValueError('A saving directory must be specified')                        # train_fcn8.py:55-56
    if pascal:
        raise NotImplementedError('pascal .mat weights are not supported')              # as buildFCN8
    if dataset not in ('camvid', 'polyps912', 'em'):
        raise ValueError('Unknown dataset')
    if dtype not in ('float32', 'float64'):
        raise NotImplementedError('training FCN-8: float32 or float64; the 16-bit legs are not trained')
    check_wgrad(wgrad, dtype)
    check_dgrad(dgrad, dtype)
    check_kxk(kxk, dtype)
    check_fwd(fwd, dtype)
    if not (isinstance(batch_size, (list, tuple)) and len(batch_size) == 3 and all(int(b) >= 1 for b in batch_size)):
        raise ValueError('batch_size must be [train, val, test], each >= 1')
    if int(num_epochs) < 1 or int(max_patience) < 1:
        raise ValueError('num_epochs and max_patience must be >= 1')
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
    exp_name = experiment_name(data_augmentation)
    loadpath = loadpath if loadpath is not None else savepath
    savepath = os.path.join(savepath, dataset, exp_name)
    loadpath = os.path.join(loadpath, dataset, exp_name)
    say = print if verbose else (lambda *a, **k: None)
    os.makedirs(savepath, exist_ok=True)
    say('Saving directory : ' + savepath)
    with open(os.path.join(savepath, 'config.txt'), 'w') as f:
        for key, value in sorted(dict(dataset=dataset, learn_step=learn_step, weight_decay=weight_decay,
                                      num_epochs=num_epochs, max_patience=max_patience,
                                      data_augmentation=data_augmentation, early_stop_class=early_stop_class,
                                      batch_size=bs, resume=resume, train_from_0_255=train_from_0_255, seed=seed,
                                      dtype=dtype, width_div=width_div, fc_channels=fc_channels,
                                      wgrad=wgrad, dgrad=dgrad, kxk=kxk, fwd=fwd).items()):
            f.write('{} = {}\n'.format(key, value))

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

    if resume:
        params = load_param_list(os.path.join(loadpath, 'new_fcn8_model_best.npz'), PARAM_ORDER)
    else:
        like = S.make_fcn8_params(nb_in_channels, n_classes, seed=1234, width_div=width_div, fc_channels=fc_channels)
        params = glorot_params({n: (like[n][0].shape, like[n][1].shape[0]) for n in PARAM_ORDER}, 4321 + int(seed))
    net = FCN8(params, n_classes, layer=['probs_dimshuffle'], dtype=tdt, mma='f32', trainable=True,
               wgrad=wgrad, dgrad=dgrad, kxk=kxk, fwd=fwd)
    trainer = FCN8Trainer(net, n_classes, void_labels, learning_rate=learn_step, weight_decay=weight_decay, seed=seed)

    def batch(it):
        X, L = it.next()
        Xd = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).cuda().to(tdt).contiguous()
        Td = torch.from_numpy(one_hot_void_last(L, n_classes)).cuda().to(tdt).contiguous()
        return Xd, Td

    def evaluate(it):
        """(mean loss, mean accuracy, Jaccard counts (2, C)) over the split: val_fn, train_fcn8.py:170-187."""
        cost = torch.zeros((), dtype=torch.float64, device='cuda')
        acc_tot, jacc_tot = 0.0, np.zeros((2, n_classes))
        for _ in range(nb(it)):
            c, m = trainer.val_step(*batch(it))
            cost += c
            acc, jacc, _ = m.result()
            acc_tot += acc
            jacc_tot += jacc
        return float(cost.item()) / nb(it), acc_tot / nb(it), jacc_tot

    def save(tag, errors):
        save_param_list(os.path.join(savepath, 'new_fcn8_model_%s.npz' % tag), net.state_arrays(), PARAM_ORDER)
        np.savez(os.path.join(savepath, 'fcn8_errors_%s.npz' % tag), *[np.asarray(e) for e in errors])

    err_train, err_valid, acc_valid, jacc_valid = [], [], [], []
    patience, best_jacc_val = 0, None
    say('Start training')
    for epoch in range(num_epochs):
        start_time = time.time()
        cost = torch.zeros((), dtype=torch.float64, device='cuda')
        for _ in range(nb(train_iter)):
            cost += trainer.train_step(*batch(train_iter))     # device scalar: one host read per epoch
        err_train.append(float(cost.item()) / nb(train_iter))

        err, acc, jacc_tot = evaluate(val_iter)
        err_valid.append(err)
        acc_valid.append(acc)
        with np.errstate(invalid='ignore', divide='ignore'):
            per_class = jacc_tot[0, :] / jacc_tot[1, :]
        jacc_valid.append(float(np.mean(per_class)) if early_stop_class is None
                          else float(per_class[int(early_stop_class)]))                 # :189-192

        out_str = 'EPOCH %i: Avg epoch training cost train %f, cost val %f, acc val %f, jacc val %f took %f s'
        out_str = out_str % (epoch, err_train[epoch], err_valid[epoch], acc_valid[epoch], jacc_valid[epoch],
                             time.time() - start_time)
        print(out_str)
        with open(os.path.join(savepath, 'fcn8_output.log'), 'a') as f:
            f.write(out_str + '\n')

        errors = (err_valid, err_train, acc_valid, jacc_valid)                          # :215-217
        if epoch == 0:                                                                  # :208-224
            best_jacc_val = jacc_valid[epoch]
        elif epoch > 1 and jacc_valid[epoch] > best_jacc_val:
            best_jacc_val = jacc_valid[epoch]
            patience = 0
            save('best', errors)
        else:
            patience += 1
            save('last', errors)

        if patience == max_patience or epoch == num_epochs - 1:                         # :227-271
            best = os.path.join(savepath, 'new_fcn8_model_best.npz')
            if test_iter is not None and os.path.exists(best):
                # the best weights back into the net's own buffer, in place
                for name, (W, b) in load_param_list(best, PARAM_ORDER).items():
                    Wd, bd = net.parameters()[name]
                    Wd.copy_(torch.from_numpy(W).to(tdt))
                    bd.copy_(torch.from_numpy(b).to(tdt))
                net.refresh()
                err, acc, jacc_tot = evaluate(test_iter)
                with np.errstate(invalid='ignore', divide='ignore'):
                    jacc = float(np.mean(jacc_tot[0, :] / jacc_tot[1, :]))
                print('FINAL MODEL: err test % f, acc test %f, jacc test %f' % (err, acc, jacc))
            elif test_iter is not None:
                # (the reference would fail here: it never wrote a best model in a run this short)
                say('no new_fcn8_model_best.npz was written: the test pass is skipped')
            if os.path.abspath(savepath) != os.path.abspath(loadpath):
                say('Copying model and other training files to {}'.format(loadpath))
                shutil.copytree(savepath, loadpath, dirs_exist_ok=True)
            break
    return {'err_train': err_train, 'err_valid': err_valid, 'acc_valid': acc_valid, 'jacc_valid': jacc_valid,
            'savepath': savepath, 'loadpath': loadpath}


def make_parser():
    parser = argparse.ArgumentParser(description='FCN-8 training')
    parser.add_argument('-dataset', default='camvid', help='Dataset.')
    parser.add_argument('-learning_rate', default=0.0001, help='Learning Rate')
    parser.add_argument('-penal_cst', default=0.0, help='regularization constant')
    parser.add_argument('--num_epochs', '-ne', type=int, default=750,
                        help='Optional. Int to indicate the max number of epochs.')
    parser.add_argument('-max_patience', type=int, default=100, help='Max patience')
    parser.add_argument('-batch_size', type=_json, default=[10, 1, 1], help='Batch size [train, val, test] (JSON)')
    parser.add_argument('-data_augmentation', type=_json, default=dict(DATA_AUGMENTATION),
                        help='use data augmentation (JSON): recorded, names the experiment folder; crop_size sets '
                             'the synthetic image size')
    parser.add_argument('-early_stop_class', type=int, default=None, help='class to early stop on')
    parser.add_argument('-train_from_0_255', type=_bool, default=False,
                        help='Whether to train from images within 0-255 range')
    parser.add_argument('-pascal', type=_bool, default=False, help='start from PASCAL .mat weights (refused)')
    parser.add_argument('--synthetic', action='store_true', help='seeded synthetic split (no dataset here)')
    parser.add_argument('--savepath', type=str, default=SAVEPATH)
    parser.add_argument('--loadpath', type=str, default=LOADPATH, help='default: --savepath')
    parser.add_argument('--resume', action='store_true', help='start from new_fcn8_model_best.npz under --loadpath')
    parser.add_argument('--dtype', default='float32', help='float32 | float64')
    parser.add_argument('--wgrad', choices=['f32', 'bf16'], default='f32',
                        help='float32: operand precision of the 3x3 weight gradients (bf16: v_mfma_f32_32x32x16_bf16 '
                             'on operands rounded once, fp32 accumulation; everything else stays float32).  Recorded '
                             'in config.txt, not in the experiment name')
    parser.add_argument('--dgrad', choices=['f32', 'bf16'], default='f32',
                        help="float32: operand precision of the backward pass's twelve 3x3 data gradients (bf16: "
                             'v_mfma_f32_32x32x16_bf16 on the parameters and g_z rounded once, fp32 accumulation).  '
                             'Recorded in config.txt, not in the experiment name')
    parser.add_argument('--kxk', choices=['f32', 'bf16'], default='f32',
                        help="float32: operand precision of fc6's and fc7's weight and data gradients (bf16: "
                             'v_mfma_f32_32x32x16_bf16 on operands rounded once, fp32 accumulation).  '
                             'Recorded in config.txt, not in the experiment name')
    parser.add_argument('--fwd', choices=['f32', 'bf16'], default='f32',
                        help="float32: operand precision of the training and validation forward's 3x3 layers, fc6 "
                             'and fc7 (bf16: v_mfma_f32_32x32x16_bf16 on operands rounded once, fp32 accumulation, '
                             'fp32 maps).  Recorded in config.txt, not in the experiment name')
    parser.add_argument('--seed', type=int, default=0, help='initial weights and the dropout generator')
    parser.add_argument('--width_div', type=int, default=1, help='divide the channel counts (small nets for tests)')
    parser.add_argument('--fc_channels', type=int, default=4096)
    parser.add_argument('--n_images', type=int, default=20, help='images per synthetic split')
    parser.add_argument('--image_size', type=int, nargs=2, default=None)
    parser.add_argument('--max_batches', type=int, default=None, help='cap on the batches of each pass (tests)')
    return parser


def parse_args(argv=None):
    return make_parser().parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    try:
        check_supported(args.dataset, args.savepath, args.pascal, args.dtype, args.batch_size, args.num_epochs,
                        args.max_patience, args.learning_rate, args.penal_cst, args.early_stop_class, args.wgrad,
                        args.dgrad, args.kxk, args.fwd)
    except (NotImplementedError, ValueError, TypeError) as e:
        print('train_fcn8.py: ' + str(e), file=sys.stderr)
        return 2
    train(args.dataset, float(args.learning_rate), float(args.penal_cst), int(args.num_epochs),
          int(args.max_patience), data_augmentation=args.data_augmentation, batch_size=args.batch_size,
          early_stop_class=args.early_stop_class, savepath=args.savepath, loadpath=args.loadpath,
          resume=args.resume, train_from_0_255=args.train_from_0_255, synthetic=args.synthetic,
          n_images=args.n_images, image_size=args.image_size, seed=args.seed, dtype=args.dtype,
          width_div=args.width_div, fc_channels=args.fc_channels, max_batches=args.max_batches, wgrad=args.wgrad,
          dgrad=args.dgrad, kxk=args.kxk, fwd=args.fwd)
    return 0


if __name__ == '__main__':
    sys.exit(main())
