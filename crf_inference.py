#!/usr/bin/env python3
"""Dense-CRF baseline on MI355X -- drop-in for the reference's crf_inference.py.

Same entry points (`inference(...)`, `main()`), same flags and defaults (`-dataset`, `-segmentation_net`,
`-which_set`, `--num_iter/-nit`, `-test_from_0_255`), same outputs: the per-class and TEST lines of
crf_inference.py:212-226, `batch%d.npz` with X, L, Y_crf, Y_fcn per batch (:201-202) and
`results_<which_set>.npz` with the per-class CRF Jaccard of every sweep entry (:257-266).  Like the
reference, `main()` ignores `--num_iter` and runs the iteration counts of its sweep (`--sweep`, default
80).  Differences, forced by the environment or deliberate:
  - the getuser() path table becomes `--savepath/--loadpath/--weights_path`; `--synthetic` supplies
    seeded data / weights when no dataset or checkpoint exists; paths are joined with separators;
  - pydensecrf's permutohedral-lattice approximation is replaced by the exact window sums of the HIP
    kernels of iterative_inference_segm_amd/crf.py (DESIGN.md "Dense-CRF baseline");
  - with -test_from_0_255 the image is read as already on 0..255 (the reference's (255 * img) overflows
    uint8 there).
"""
import argparse
import os
import shutil

import numpy as np
import torch

from iterative_inference_segm_amd import synthetic as S
from iterative_inference_segm_amd.api import IterativeInference
from iterative_inference_segm_amd.crf import DenseCRF
from iterative_inference_segm_amd.data_loader import load_data
from iterative_inference_segm_amd.fcn8 import buildFCN8

SAVEPATH = os.environ.get('IISEG_SAVEPATH', './iiseg_out/save/')
LOADPATH = os.environ.get('IISEG_LOADPATH', './iiseg_out/load/')
WEIGHTS_PATH = os.environ.get('IISEG_WEIGHTS_PATH', './iiseg_out/load/')

BATCH_SIZE = 10   # crf_inference.py:56-57


def build_segmentation_net(segm_net, dataset, weights_path, n_classes, nb_in_channels, synthetic,
                           device='cuda'):
    """FCN-8 (crf_inference.py:74-80; fcn8_void appends a zero void channel) or FC-DenseNet103 (:81-84)."""
    if segm_net == 'fcn8':
        path = os.path.join(weights_path, dataset, 'fcn8_model.npz')
        params = None
        if not os.path.exists(path):
            if not synthetic:
                raise IOError('FCN-8 weights not found: %s (use --synthetic)' % path)
            params = S.make_fcn8_params(nb_in_channels, n_classes, seed=1234)
        return buildFCN8(nb_in_channels, path_weights=path, n_classes=n_classes, trainable=False,
                         load_weights=True, layer=['probs_dimshuffle'], params=params, device=device)
    if segm_net == 'densenet':
        from iterative_inference_segm_amd.densenet import build_fcdensenet, layer_plan
        path = os.path.join(weights_path, dataset, 'FC-DenseNet103_weights.npz')
        params = None
        if not os.path.exists(path):
            if not synthetic:
                raise IOError('FC-DenseNet weights not found: %s (use --synthetic)' % path)
            params = S.make_densenet_params(layer_plan(nb_in_channels=nb_in_channels, n_classes=n_classes),
                                            seed=2024)
        return build_fcdensenet(layer=[], nb_in_channels=nb_in_channels, n_classes=n_classes,
                                weight_path=path, params=params, device=device)
    if segm_net == 'fcn_fcresnet':
        raise NotImplementedError                                      # :85-86
    raise ValueError('Unknown segmentation net %r' % (segm_net,))      # :87-88


def inference(dataset, segm_net, which_set='val', num_iter=5, Bilateral=True, savepath=None,
              loadpath=None, test_from_0_255=False, weights_path=None, synthetic=False, n_images=20,
              image_size=(224, 224), batch_size=BATCH_SIZE, crf=None, verbose=True):
    """Signature of reference crf_inference.py:44-45 plus keyword extras.  Returns the per-class CRF
    Jaccard (n_classes,) as the reference does."""
    say = print if verbose else (lambda *a, **k: None)
    if savepath is None:
        raise ValueError('A saving directory must be specified')
    loadpath = loadpath if loadpath is not None else LOADPATH
    weights_path = weights_path if weights_path is not None else WEIGHTS_PATH

    # Build dataset iterator (:56-62)
    data_iter = load_data(dataset, {}, one_hot=True, batch_size=[batch_size] * 3,
                          return_0_255=test_from_0_255, which_set=which_set, synthetic=synthetic,
                          n_images=n_images, image_size=image_size)
    n_batches_test = data_iter.nbatches
    n_classes = data_iter.non_void_nclasses
    void_labels = data_iter.void_labels

    # Prepare saving directory (:67-71)
    savepath = os.path.join(savepath, dataset, segm_net, 'img_plots', 'crf', str(num_iter), which_set)
    loadpath = os.path.join(loadpath, dataset, segm_net, 'img_plots', 'crf', str(num_iter), which_set)
    if not os.path.exists(savepath):
        os.makedirs(savepath)

    # Build network (:73-88)
    say('Building segmentation network')
    device = 'cuda'
    fcn = build_segmentation_net(segm_net, dataset, weights_path, n_classes, data_iter.data_shape[0],
                                 synthetic, device)
    ii = IterativeInference(fcn, None, n_classes, void_labels, device=device)
    crf = DenseCRF() if crf is None else crf

    say('Start infering')
    acc_tot_crf = acc_tot_fcn = 0.0
    jacc_tot_crf = np.zeros((2, n_classes))
    jacc_tot_fcn = np.zeros((2, n_classes))
    for i in range(n_batches_test):
        say('Batch %d out of %d' % (i + 1, n_batches_test))
        X_test_batch, L_test_batch = data_iter.batch(i) if hasattr(data_iter, 'batch') else data_iter.next()
        L_test_batch = L_test_batch.astype(np.float32)
        X_dev = torch.from_numpy(np.ascontiguousarray(X_test_batch, dtype=np.float32)).to(device)
        L_dev = torch.from_numpy(L_test_batch).to(device)

        # segmentation net (:128-133) and its metrics
        out = ii.pred_fcn_fn(X_dev)
        P = (out[-1] if isinstance(out, (list, tuple)) else out)[:, :n_classes].contiguous()
        acc_fcn, jacc_fcn, _ = ii.val_fn(P, L_dev)
        acc_tot_fcn += acc_fcn
        jacc_tot_fcn += jacc_fcn

        # CRF on the whole batch (:143-180) and its metrics (:185-188)
        Q = crf.inference(P, X_dev, num_iter, bilateral=Bilateral, input_0_255=test_from_0_255)
        acc_crf, jacc_crf, _ = ii.val_fn(Q, L_dev)
        acc_tot_crf += acc_crf
        jacc_tot_crf += jacc_crf

        Y_fcn = P.cpu().numpy()
        if segm_net == 'fcn8' and void_labels:
            # fcn8_void's output: the class probabilities and a zero void channel (models/fcn8_void.py:139-147)
            Y_fcn = np.concatenate([Y_fcn, np.zeros_like(Y_fcn[:, :1])], axis=1)
        np.savez(os.path.join(savepath, 'batch' + str(i) + '.npz'), X=X_test_batch, L=L_test_batch,
                 Y_crf=Q.cpu().numpy(), Y_fcn=Y_fcn)

    acc_test_crf = acc_tot_crf / n_batches_test
    with np.errstate(invalid='ignore', divide='ignore'):
        jacc_test_perclass_crf = jacc_tot_crf[0, :] / jacc_tot_crf[1, :]
        jacc_test_perclass_fcn = jacc_tot_fcn[0, :] / jacc_tot_fcn[1, :]
    jacc_test_crf = np.nanmean(jacc_test_perclass_crf)
    acc_test_fcn = acc_tot_fcn / n_batches_test
    jacc_test_fcn = np.nanmean(jacc_test_perclass_fcn)

    out_str = 'TEST: acc crf %f, jacc crf %f, acc fcn %f, jacc fcn %f' % (
        acc_test_crf, jacc_test_crf, acc_test_fcn, jacc_test_fcn)
    say('>>>>> Per class jaccard:')
    labs = data_iter.mask_labels
    for c in range(len(labs) - len(void_labels)):
        say('    ' + labs[c] + ' : fcn ->  %f, crf ->  %f' % (jacc_test_perclass_fcn[c], jacc_test_perclass_crf[c]))
    say(out_str)

    # Move segmentations (:229-232)
    if savepath != loadpath:
        say('Copying images to {}'.format(loadpath))
        shutil.copytree(savepath, loadpath, dirs_exist_ok=True)
    return jacc_test_perclass_crf


def main(argv=None):
    parser = argparse.ArgumentParser(description='Unet model training')
    parser.add_argument('-dataset', type=str, default='camvid', help='Dataset.')
    parser.add_argument('-segmentation_net', type=str, default='fcn8', help='Segmentation network.')
    parser.add_argument('-which_set', type=str, default='test', help='Step')
    parser.add_argument('--num_iter', '-nit', type=int, default=10,
                        help='Max number of iterations (ignored, as in the reference: see --sweep).')
    parser.add_argument('-test_from_0_255', type=bool, default=False,
                        help='Whether to train from images within 0-255 range')
    # the iteration counts main() runs (the reference hard-codes num_iter = [80], crf_inference.py:257)
    parser.add_argument('--sweep', type=int, nargs='+', default=[80],
                        help='mean-field iteration counts to evaluate (default 80)')
    # replacements for the getuser() path table, and synthetic mode
    parser.add_argument('--savepath', type=str, default=SAVEPATH)
    parser.add_argument('--loadpath', type=str, default=LOADPATH)
    parser.add_argument('--weights_path', type=str, default=WEIGHTS_PATH)
    parser.add_argument('--synthetic', action='store_true',
                        help='seeded synthetic data and weights (no dataset / checkpoints here)')
    parser.add_argument('--n_images', type=int, default=20)
    parser.add_argument('--image_size', type=int, nargs=2, default=[224, 224])
    args = parser.parse_args(argv)

    sp = os.path.join(args.loadpath, args.dataset, args.segmentation_net, 'img_plots', 'crf')
    valid_mat = None
    for i, val_i in enumerate(args.sweep):
        res = inference(args.dataset, args.segmentation_net, which_set=args.which_set, num_iter=val_i,
                        savepath=args.savepath, loadpath=args.loadpath,
                        test_from_0_255=args.test_from_0_255, weights_path=args.weights_path,
                        synthetic=args.synthetic, n_images=args.n_images,
                        image_size=tuple(args.image_size))
        if valid_mat is None:
            valid_mat = np.zeros((len(res), len(args.sweep)))
        valid_mat[:, i] = res
    os.makedirs(sp, exist_ok=True)
    np.savez(os.path.join(sp, 'results_' + args.which_set + '.npz'), valid_mat)
    return valid_mat


if __name__ == '__main__':
    main()
