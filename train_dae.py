#!/usr/bin/env python3
"""Training the DAE on MI355X -- counterpart of the reference's train_dae.py for the DAE kind it defaults to,
'contextmod' (train_dae.py:479-488), and for kind 'standard' with h at a pool point (e.g. -dae_dict
'{"kind": "standard", "concat_h": ["pool4"]}' -segmentation_net fcn8; checkpoint in dae.param_order).

Same arguments and defaults (`-dataset`, `-segmentation_net`, `-train_dict`, `-dae_dict`,
`-data_augmentation`, `-train_from_0_255`; the dict arguments are JSON), the same epoch loop
(train_dae.py:351-457: training pass, validation pass, lr <- lr * lr_anneal, early stopping on the
validation loss with `max_patience`), the same files in the experiment folder named by
helpers.build_experiment_name: `dae_model_best.npz` / `dae_model_last.npz` (np.savez of W, b per layer in
contextmod.PARAM_ORDER), `dae_errors_best.npz` / `dae_errors_last.npz`, `output.log`, `config.txt`.
The lab paths keyed on getuser() become `--savepath / --loadpath / --weights_path`; `--synthetic` supplies the
seeded synthetic split and initial weights.  What is not built is refused before any GPU work, with the
reason: kind 'fcn8', kind 'standard' with bn / dropout / conv_before_pool != 1 / unpool_type 'standard' or with
the image concatenated at the input, the 'dice' and 'squared_error_h' losses, `ae_h`, `full_im_ft`.
All arithmetic runs in the HIP kernels of libiiseg_hip.so.
`--wgrad bf16` (kind 'standard', float32 only) forms the 3x3 weight gradients on the 16-bit
matrix pipe from operands rounded once to bf16; the forward, the data gradients, the parameters, the optimizer
state and the checkpoints stay float32, so the experiment folder keeps its name (config.txt records the mode).
With `--dtype float64` or kind 'contextmod' it is refused before any GPU work.
`--dgrad bf16` (the same conditions and refusals) forms the 3x3 data gradients of the backward
pass on the 16-bit matrix pipe from the parameters and g_z rounded once to bf16; config.txt records it as well.
`-train_dict '{"fwd": "bf16"}'` (the same conditions and refusals) runs every forward of the
standard DAE -- training, validation -- on the 16-bit matrix pipe from W and the layer inputs rounded once to bf16;
it has no flag of its own and is no default of the dictionary; config.txt records it as well.
"""
import argparse
import json
import os
import shutil
import sys
import time

import numpy as np

from iterative_inference_segm_amd.helpers import build_experiment_name

SAVEPATH = os.environ.get('IISEG_SAVEPATH', './iiseg_out/save/')
LOADPATH = os.environ.get('IISEG_LOADPATH', './iiseg_out/load/')
WEIGHTS_PATH = os.environ.get('IISEG_WEIGHTS_PATH', './iiseg_out/load/')

TRAIN_DICT = {'learning_rate': 0.0001, 'lr_anneal': 0.99, 'weight_decay': 0.0001, 'num_epochs': 500,
              'max_patience': 100, 'optimizer': 'rmsprop', 'batch_size': [10, 10, 10],
              'training_loss': ['crossentropy'], 'lmb': 1, 'full_im_ft': False}          # train_dae.py:472-477
DAE_DICT = {'kind': 'contextmod', 'dropout': 0, 'skip': True, 'unpool_type': 'trackind', 'noise': 0,
            'concat_h': ['input'], 'from_gt': False, 'n_filters': 64, 'conv_before_pool': 1,
            'additional_pool': 2, 'temperature': 1.0, 'path_weights': '', 'layer': 'probs_dimshuffle',
            'exp_name': 'flip_final_', 'bn': 0}                                            # :481-487
DATA_AUGMENTATION = {'crop_size': [224, 224], 'horizontal_flip': 0.5, 'fill_mode': 'constant'}   # :491-494


def _json_dict(s):
    return json.loads(s) if isinstance(s, str) else s


def check_supported(dae_dict, training_loss, ae_h, full_im_ft, optimizer, wgrad='f32', dtype='float32',
                    dgrad='f32', fwd='f32'):
    """Everything this build does not train, refused with the reason (host only)."""
    from iterative_inference_segm_amd.train import check_supported as chk
    chk(dae_dict['kind'], training_loss, ae_h, full_im_ft, optimizer, dae_dict=dae_dict, wgrad=wgrad, dtype=dtype,
        dgrad=dgrad, fwd=fwd)
    if dae_dict['kind'] == 'contextmod' and list(dae_dict['concat_h']) != ['input']:
        raise NotImplementedError("the context module concatenates the image: concat_h must be ['input']")


def save_checkpoint(savepath, tag, params, errors, order=None):
    """dae_model_<tag>.npz (weights.save_param_list in `order`, default contextmod.PARAM_ORDER: what
    np.savez(*get_all_param_values(dae)) wrote, train_dae.py:436-445) and dae_errors_<tag>.npz."""
    from iterative_inference_segm_amd.contextmod import PARAM_ORDER
    from iterative_inference_segm_amd.weights import save_param_list
    save_param_list(os.path.join(savepath, 'dae_model_%s.npz' % tag), params, order or PARAM_ORDER)
    np.savez(os.path.join(savepath, 'dae_errors_%s.npz' % tag), *[np.asarray(e) for e in errors])


def build_segmentation_net(dataset, segm_net, dae_dict, weights_path, n_classes, void_labels, nb_in_channels,
                           synthetic):
    """fcn_fn(X) -> [H..., Y] of train_dae.py:154-172,337: the frozen segmentation net alone."""
    from iterative_inference_segm_amd import synthetic as S
    layers = list(dae_dict['concat_h']) + [dae_dict['layer']]
    if segm_net == 'fcn8':
        from iterative_inference_segm_amd.fcn8 import buildFCN8
        path = os.path.join(weights_path, dataset, 'fcn8_model.npz')
        params = None
        if not os.path.exists(path):
            if not synthetic:
                raise IOError('FCN-8 weights not found: %s (use --synthetic)' % path)
            params = S.make_fcn8_params(nb_in_channels, n_classes, seed=1234)
        return buildFCN8(nb_in_channels, path_weights=path, n_classes=n_classes, void_labels=void_labels,
                         trainable=False, load_weights=True, layer=layers, params=params)
    from iterative_inference_segm_amd.densenet import build_fcdensenet, layer_plan
    path = os.path.join(weights_path, dataset, 'FC-DenseNet103_weights.npz')
    params = None
    if not os.path.exists(path):
        if not synthetic:
            raise IOError('FC-DenseNet weights not found: %s (use --synthetic)' % path)
        params = S.make_densenet_params(layer_plan(nb_in_channels=nb_in_channels, n_classes=n_classes), seed=2024)
    return build_fcdensenet(layer=dae_dict['concat_h'], nb_in_channels=nb_in_channels, n_classes=n_classes,
                            weight_path=path, params=params)


def train(dataset, segm_net, learning_rate=0.005, lr_anneal=1.0, weight_decay=1e-4, num_epochs=500,
          max_patience=100, optimizer='rmsprop', training_loss=['squared_error'], batch_size=[10, 1, 1],
          ae_h=False, dae_dict_updates={}, data_augmentation={}, savepath=None, loadpath=None, resume=False,
          train_from_0_255=False, lmb=1, full_im_ft=False, weights_path=None, synthetic=False, n_images=20,
          image_size=None, seed=0, dtype='float32', wgrad='f32', dgrad='f32', fwd='f32', verbose=True):
    """Signature of reference train_dae.py:54-60 plus keyword-only extras.  weight_decay only enters the
    experiment name, as in the reference (train_dae.py:91: no regulariser is added to the loss).  wgrad (kind
    'standard': 'f32' | 'bf16', the 3x3 weight gradients' operand precision) is recorded in config.txt and stays
    out of the experiment name: the checkpoints are float32 either way; dgrad (the 3x3 data gradients') and fwd
    (every forward of the module: StandardDAE's `fwd`) likewise.
    Returns the
    per-epoch lists (err_train, err_valid, jacc_val, mse_val) and the experiment folder."""
    dae_dict = {'kind': 'fcn8', 'dropout': 0.0, 'skip': True, 'unpool_type': 'standard', 'n_filters': 64,
                'conv_before_pool': 1, 'additional_pool': 0, 'concat_h': ['input'], 'noise': 0.0,
                'from_gt': True, 'temperature': 1.0, 'path_weights': '', 'layer': 'probs_dimshuffle',
                'exp_name': '', 'bn': 0}                                                  # :65-79
    dae_dict.update(dae_dict_updates)
    check_supported(dae_dict, training_loss, ae_h, full_im_ft, optimizer, wgrad, dtype, dgrad, fwd)
    if dataset not in ('camvid', 'polyps912', 'em'):
        raise ValueError('Unknown dataset')
    if segm_net == 'fcn_fcresnet':
        raise NotImplementedError
    if segm_net not in ('fcn8', 'densenet'):
        raise ValueError('Unknown segmentation network')

    exp_name = build_experiment_name(segm_net, training_loss=training_loss, data_aug=bool(data_augmentation),
                                     learning_rate=learning_rate, lr_anneal=lr_anneal,
                                     weight_decay=weight_decay, optimizer=optimizer, ae_h=ae_h, **dae_dict)
    if savepath is None:
        raise ValueError('A saving directory must be specified')
    loadpath = loadpath if loadpath is not None else LOADPATH
    weights_path = weights_path if weights_path is not None else WEIGHTS_PATH
    loadpath_init = os.path.join(loadpath, dataset, exp_name)
    loadpath = os.path.join(loadpath, dataset, exp_name)
    savepath = os.path.join(savepath, dataset, exp_name)
    say = print if verbose else (lambda *a, **k: None)
    os.makedirs(savepath, exist_ok=True)
    say('Saving directory : ' + savepath)
    with open(os.path.join(savepath, 'config.txt'), 'w') as f:
        for key, value in sorted(dict(dataset=dataset, segm_net=segm_net, learning_rate=learning_rate,
                                      lr_anneal=lr_anneal, weight_decay=weight_decay, num_epochs=num_epochs,
                                      max_patience=max_patience, optimizer=optimizer,
                                      training_loss=training_loss, batch_size=batch_size, dae_dict=dae_dict,
                                      data_augmentation=data_augmentation, resume=resume, lmb=lmb,
                                      train_from_0_255=train_from_0_255, seed=seed, dtype=dtype,
                                      wgrad=wgrad, dgrad=dgrad, fwd=fwd).items()):
            f.write('{} = {}\n'.format(key, value))

    # ---- from here on: the GPU ----
    import torch
    from iterative_inference_segm_amd import synthetic as S
    from iterative_inference_segm_amd.contextmod import PARAM_ORDER, buildDAE_contextmod
    from iterative_inference_segm_amd.data_loader import load_data
    from iterative_inference_segm_amd.train import DAETrainer
    from iterative_inference_segm_amd.weights import load_param_list

    tdt = {'float32': torch.float32, 'float64': torch.float64}[dtype]
    crop = (data_augmentation or {}).get('crop_size')
    size = tuple(image_size) if image_size is not None else (tuple(crop) if crop else (360, 480))
    train_iter, val_iter, _ = load_data(dataset, data_augmentation, one_hot=True, batch_size=batch_size,
                                        return_0_255=train_from_0_255, synthetic=True if synthetic else None,
                                        n_images=n_images, image_size=size)
    n_classes, void_labels = train_iter.non_void_nclasses, train_iter.void_labels
    nb_in_channels = train_iter.data_shape[0]
    void = n_classes if any(void_labels) else n_classes + 1

    fcn_fn = None
    if not dae_dict['from_gt'] or dae_dict['kind'] == 'standard':       # (the standard kind's h: its feature maps)
        say('Building segmentation network')
        fcn_fn = build_segmentation_net(dataset, segm_net, dae_dict, weights_path, n_classes, void_labels,
                                        nb_in_channels, synthetic)

    say('Building DAE network')
    init = os.path.join(loadpath_init, 'dae_model_best.npz')
    standard = dae_dict['kind'] == 'standard'
    if standard:
        from iterative_inference_segm_amd.dae import StandardDAE, param_order
        arch = dict(concat_h=list(dae_dict['concat_h']), conv_before_pool=dae_dict['conv_before_pool'],
                    additional_pool=dae_dict['additional_pool'], unpool_type=dae_dict['unpool_type'])
        order = param_order(bn=0, **arch)
        if resume:
            params = load_param_list(init, order)
        else:
            # channels of the h maps: one forward of the frozen net on a blank image
            probe = torch.zeros((1, nb_in_channels) + tuple(size), dtype=torch.float32, device='cuda')
            h_channels = tuple(int(h.shape[1]) for h in fcn_fn(probe)[:-1])
            params = S.make_dae_params(n_classes, h_channels, n_filters=dae_dict['n_filters'],
                                       seed=4321 + int(seed), **arch)
        dae = StandardDAE(params, n_classes, padding=100, n_filters=dae_dict['n_filters'],
                          skip=dae_dict['skip'], noise=dae_dict['noise'], dtype=tdt, mma='f32', trainable=True,
                          wgrad=wgrad, dgrad=dgrad, fwd=fwd, **arch)
    else:
        order = PARAM_ORDER
        if resume:
            params = load_param_list(init, PARAM_ORDER)
        else:
            params = S.make_contextmod_params(n_classes, nb_in_channels, seed=777 + int(seed))
        dae = buildDAE_contextmod(n_classes=n_classes, trainable=True, noise=dae_dict['noise'],
                                  concat_h=dae_dict['concat_h'], params=params, dtype=tdt)
    trainer = DAETrainer(fcn_fn, dae, n_classes, void_labels, optimizer=optimizer, learning_rate=learning_rate,
                         training_loss=training_loss, lmb=lmb, noise=float(dae_dict['noise']), seed=seed)

    def batch(it):
        X, L = it.next()
        Xd = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).cuda()
        Ld = torch.from_numpy(np.ascontiguousarray(L)).cuda().to(tdt).contiguous()
        if dae_dict['from_gt']:
            Y = Ld[:, :void].contiguous()                                               # :371-372
        elif not standard:
            Y = fcn_fn(Xd)[-1].to(tdt).contiguous()                                     # :374
        else:
            Y = None
        if standard:
            out = fcn_fn(Xd)
            H = [h.to(tdt).contiguous() for h in out[:-1]]
            return H, (Y if dae_dict['from_gt'] else out[-1].to(tdt).contiguous()), Ld
        return Xd.to(tdt).contiguous(), Y, Ld

    err_train, err_valid, jacc_val_arr, mse_val_arr = [], [], [], []
    patience = 0
    best_err_val = None
    say('Start training')
    for epoch in range(num_epochs):
        start_time = time.time()
        cost = torch.zeros((), dtype=torch.float64, device='cuda')
        for _ in range(train_iter.nbatches):
            H, Y, L = batch(train_iter)
            cost += trainer.train_step(H, Y, L)            # device scalar: one host read per epoch
        err_train.append(float(cost.item()) / train_iter.nbatches)

        cost = torch.zeros((), dtype=torch.float64, device='cuda')
        mse = torch.zeros((), dtype=torch.float64, device='cuda')
        jacc_tot = np.zeros((2, n_classes))
        for _ in range(val_iter.nbatches):
            H, Y, L = batch(val_iter)
            c, m, e = trainer.val_step(H, Y, L)
            cost += c
            mse += e
            jacc_tot += m.result()[1]
        err_valid.append(float(cost.item()) / val_iter.nbatches)
        with np.errstate(invalid='ignore', divide='ignore'):
            jacc_val_arr.append(float(np.mean(jacc_tot[0, :] / jacc_tot[1, :])))       # :408
        mse_val_arr.append(float(mse.item()) / val_iter.nbatches)

        out_str = 'EPOCH %i: Avg epoch training cost train %f, cost val %f, jacc val %f, mse val % f took %f s'
        out_str = out_str % (epoch, err_train[epoch], err_valid[epoch], jacc_val_arr[epoch], mse_val_arr[epoch],
                             time.time() - start_time)
        print(out_str)
        with open(os.path.join(savepath, 'output.log'), 'a') as f:
            f.write(out_str + '\n')

        trainer.anneal(lr_anneal)                                                       # :424

        errors = (err_train, err_valid, jacc_val_arr, mse_val_arr)
        if epoch == 0:                                                                  # :427-445
            best_err_val = err_valid[epoch]
            # the reference writes no checkpoint for epoch 0; this build does, so that a run of one epoch
            # leaves a model behind
            save_checkpoint(savepath, 'best', dae.state_arrays(), errors, order)
        elif err_valid[epoch] < best_err_val:
            best_err_val = err_valid[epoch]
            patience = 0
            save_checkpoint(savepath, 'best', dae.state_arrays(), errors, order)
        else:
            patience += 1
            save_checkpoint(savepath, 'last', dae.state_arrays(), errors, order)

        if patience == max_patience or epoch == num_epochs - 1:
            save_checkpoint(savepath, 'last', dae.state_arrays(), errors, order)
            if os.path.abspath(savepath) != os.path.abspath(loadpath):
                say('Copying model and other training files to {}'.format(loadpath))
                shutil.copytree(savepath, loadpath, dirs_exist_ok=True)
            say(' Training Done !')
            break
    return {'err_train': err_train, 'err_valid': err_valid, 'jacc_val': jacc_val_arr, 'mse_val': mse_val_arr,
            'savepath': savepath, 'loadpath': loadpath}


def make_parser():
    parser = argparse.ArgumentParser(description='DAE training')
    parser.add_argument('-dataset', type=str, default='camvid', help='Dataset.')
    parser.add_argument('-segmentation_net', type=str, default='densenet', help='Segmentation network.')
    parser.add_argument('-train_dict', type=_json_dict, default=dict(TRAIN_DICT),
                        help='Training configuration (JSON; keys given replace the defaults).  weight_decay '
                             'only enters the experiment name, as in the reference: no regulariser is added '
                             'to the loss.  "fwd": "bf16" (kind \'standard\', float32; no default of the dictionary '
                             'and no flag of its own) runs the DAE\'s forward on the 16-bit matrix pipe: recorded in '
                             'config.txt, not in the experiment name')
    parser.add_argument('-dae_dict', type=_json_dict, default=dict(DAE_DICT),
                        help="DAE kind and parameters (JSON).  Kinds 'contextmod' and 'standard' (h at a pool point) are "
                             "trained here")
    parser.add_argument('-data_augmentation', type=_json_dict, default=dict(DATA_AUGMENTATION),
                        help='Dictionary of data augmentation (JSON): accepted and recorded in the experiment '
                             'name; crop_size sets the synthetic image size')
    parser.add_argument('-train_from_0_255', type=lambda s: str(s).lower() in ('1', 'true', 'yes'),
                        default=False, help='Whether to train from images within 0-255 range')
    parser.add_argument('-ae_h', type=lambda s: str(s).lower() in ('1', 'true', 'yes'), default=False,
                        help='Plug&Play DAE on h (refused: not built)')
    parser.add_argument('--synthetic', action='store_true',
                        help='seeded synthetic split and initial weights (no dataset here)')
    parser.add_argument('--savepath', type=str, default=SAVEPATH)
    parser.add_argument('--loadpath', type=str, default=LOADPATH)
    parser.add_argument('--weights_path', type=str, default=WEIGHTS_PATH)
    parser.add_argument('--resume', action='store_true', help='start from dae_model_best.npz under --loadpath')
    parser.add_argument('--num_epochs', type=int, default=None, help='overrides train_dict.num_epochs')
    parser.add_argument('--seed', type=int, default=0, help='initial weights and the noise generator')
    parser.add_argument('--n_images', type=int, default=20, help='images per synthetic split')
    parser.add_argument('--image_size', type=int, nargs=2, default=None)
    parser.add_argument('--dtype', choices=['float32', 'float64'], default='float32')
    parser.add_argument('--wgrad', choices=['f32', 'bf16'], default='f32',
                        help="kind 'standard', float32: operand precision of the 3x3 weight gradients (bf16: "
                             'v_mfma_f32_32x32x16_bf16 on operands rounded once, fp32 accumulation; everything '
                             'else stays float32).  Recorded in config.txt, not in the experiment name')
    parser.add_argument('--dgrad', choices=['f32', 'bf16'], default='f32',
                        help="kind 'standard', float32: operand precision of the backward pass's 3x3 data gradients "
                             '(bf16: v_mfma_f32_32x32x16_bf16 on the parameters and g_z rounded once, fp32 '
                             'accumulation).  Recorded in config.txt, not in the experiment name')
    return parser


def parse_args(argv=None):
    """(args, train_dict, dae_dict): the dict options merged over the reference's defaults."""
    args = make_parser().parse_args(argv)
    train_dict = dict(TRAIN_DICT)
    train_dict.update(args.train_dict)
    dae_dict = dict(DAE_DICT)
    dae_dict.update(args.dae_dict)
    if args.num_epochs is not None:
        train_dict['num_epochs'] = int(args.num_epochs)
    return args, train_dict, dae_dict


def main(argv=None):
    args, train_dict, dae_dict = parse_args(argv)
    try:
        check_supported(dae_dict, train_dict['training_loss'], args.ae_h, train_dict.get('full_im_ft', False),
                        train_dict['optimizer'], args.wgrad, args.dtype, args.dgrad,
                        train_dict.get('fwd', 'f32'))
    except (NotImplementedError, ValueError) as e:
        print('train_dae.py: ' + str(e), file=sys.stderr)
        return 2
    train(dataset=args.dataset, segm_net=args.segmentation_net, dae_dict_updates=dae_dict, ae_h=args.ae_h,
          data_augmentation=args.data_augmentation, train_from_0_255=args.train_from_0_255, resume=args.resume,
          savepath=args.savepath, loadpath=args.loadpath, weights_path=args.weights_path,
          synthetic=args.synthetic, n_images=args.n_images, image_size=args.image_size, seed=args.seed,
          dtype=args.dtype, wgrad=args.wgrad, dgrad=args.dgrad, **train_dict)
    return 0


if __name__ == '__main__':
    sys.exit(main())
