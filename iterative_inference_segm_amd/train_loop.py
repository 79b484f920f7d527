"""What train_fcn8.py and train_fcdensenet.py share: the common options and refusals, the
experiment folder, one validation pass, and the epoch loop of the reference's train_fcn8.py:150-271 with its best /
last / patience rule as a function of its own.  Host code: importing it loads numpy and no torch (to_device,
train_steps and evaluate import it when called), so the options, the refusals, the loop and its rules run without it."""
import argparse
import json
import os
import shutil
import sys
import time

import numpy as np

from .params import MODES_16BIT, SWITCHES_16BIT, check_mode

DATASETS = ('camvid', 'polyps912', 'em')
LOG_LINE = 'EPOCH %i: Avg epoch training cost train %f, cost val %f, acc val %f, jacc val %f took %f s'


def json_arg(s):
    return json.loads(s) if isinstance(s, str) else s


def one_hot_void_last(L, n_classes):
    """Integer labels (B,H,W), void = any label >= n_classes, -> one-hot (B,n_classes+1,H,W), void channel last."""
    L = np.minimum(np.asarray(L).astype(np.int64), n_classes)
    return np.ascontiguousarray(np.moveaxis(np.eye(n_classes + 1, dtype=np.float32)[L], -1, 1))


# ---- the command line ----
def add_switch(parser, switch, of):
    """The option of one 16-bit training switch (params.SWITCHES_16BIT); of: the layers it covers in this net."""
    parser.add_argument('--' + switch, choices=list(MODES_16BIT), default='f32',
                        help='operand precision of the %s: %s (bf16: float32 runs only, operands rounded once, '
                             'fp32 accumulation); recorded in config.txt' % (SWITCHES_16BIT[switch], of))


def make_parser(description, switches):
    """The options both drivers have; switches: {switch: the layers it covers}."""
    parser = argparse.ArgumentParser(description=description)
    parser.add_argument('-dataset', default='camvid', help='Dataset.')
    parser.add_argument('--num_epochs', '-ne', type=int, default=750, help='the max number of epochs')
    parser.add_argument('--synthetic', action='store_true', help='seeded synthetic split (no dataset here)')
    parser.add_argument('--savepath', type=str, default=os.environ.get('IISEG_SAVEPATH'))
    parser.add_argument('--loadpath', type=str, default=os.environ.get('IISEG_LOADPATH'), help='default: --savepath')
    parser.add_argument('--resume', action='store_true', help='start from the best checkpoint under --loadpath')
    parser.add_argument('--dtype', default='float32', help='float32 | float64')
    for switch, of in switches.items():
        add_switch(parser, switch, of)
    parser.add_argument('--seed', type=int, default=0, help='initial weights and the dropout generator')
    parser.add_argument('--n_images', type=int, default=20, help='images per synthetic split')
    parser.add_argument('--image_size', type=int, nargs=2, default=None)
    parser.add_argument('--max_batches', type=int, default=None, help='cap on the batches of each pass (tests)')
    return parser


def check_savepath(savepath):
    if savepath is None:
        raise ValueError('A saving directory must be specified')                        # train_fcn8.py:55-56


def check_dataset(dataset):
    if dataset not in DATASETS:
        raise ValueError('Unknown dataset')


def check_switches(dtype, **modes):
    """Each 16-bit switch's mode, refused where a run of precision `dtype` has no such form."""
    for switch, mode in modes.items():
        check_mode(switch, mode, dtype)


def check_schedule(batch_size, num_epochs, max_patience):
    if not (isinstance(batch_size, (list, tuple)) and len(batch_size) == 3 and all(int(b) >= 1 for b in batch_size)):
        raise ValueError('batch_size must be [train, val, test], each >= 1')
    if int(num_epochs) < 1 or int(max_patience) < 1:
        raise ValueError('num_epochs and max_patience must be >= 1')


def main(script, check, run):
    """What is refused exits with status 2 and the reason on stderr, before any GPU work."""
    try:
        check()
    except (NotImplementedError, ValueError, TypeError) as e:
        print('%s: %s' % (script, e), file=sys.stderr)
        return 2
    run()
    return 0


# ---- the experiment folder ----
def experiment_folders(savepath, loadpath, dataset, exp_name, config, say=print):
    """(savepath, loadpath)/<dataset>/<exp_name>, the first created with `config` in its config.txt."""
    loadpath = loadpath if loadpath is not None else savepath
    savepath = os.path.join(savepath, dataset, exp_name)
    loadpath = os.path.join(loadpath, dataset, exp_name)
    os.makedirs(savepath, exist_ok=True)
    say('Saving directory : ' + savepath)
    with open(os.path.join(savepath, 'config.txt'), 'w') as f:
        for key, value in sorted(config.items()):
            f.write('{} = {}\n'.format(key, value))
    return savepath, loadpath


# ---- the device side of a pass ----
def to_device(batch, n_classes, dtype):
    """(X, integer labels) of an iterator -> (X, one-hot T with void last) on the device in `dtype`, the net's."""
    import torch
    X, L = batch
    return (torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).cuda().to(dtype).contiguous(),
            torch.from_numpy(one_hot_void_last(L, n_classes)).cuda().to(dtype).contiguous())


def train_steps(trainer, it, nb, n_classes):
    """The summed cost of `nb` training steps, a device scalar: the loop reads it once per epoch."""
    import torch
    cost = torch.zeros((), dtype=torch.float64, device='cuda')
    for _ in range(nb):
        cost += trainer.train_step(*to_device(it.next(), n_classes, trainer.net.flat.dtype))
    return cost


def evaluate(trainer, it, nb, n_classes):
    """(mean loss, mean accuracy, Jaccard counts (2, C)) over `nb` batches: val_fn, train_fcn8.py:170-187."""
    import torch
    cost = torch.zeros((), dtype=torch.float64, device='cuda')
    acc_tot, jacc_tot = 0.0, np.zeros((2, n_classes))
    for _ in range(nb):
        c, m = trainer.val_step(*to_device(it.next(), n_classes, trainer.net.flat.dtype))
        cost += c
        acc, jacc, _ = m.result()
        acc_tot += acc
        jacc_tot += jacc
    return float(cost.item()) / nb, acc_tot / nb, jacc_tot


def per_class_jaccard(jacc_tot):
    """Intersection over union per class; NaN for a class the split does not show."""
    with np.errstate(invalid='ignore', divide='ignore'):
        return jacc_tot[0, :] / jacc_tot[1, :]


# ---- the loop ----
def fcn8_rule(epoch, value, best):
    """train_fcn8.py:208-224: epoch 0 sets the best value and saves nothing, epoch 1 is never the best."""
    if epoch == 0:
        return True, None
    return (True, 'best') if epoch > 1 and value > best else (False, 'last')


def first_epoch_best_rule(epoch, value, best):
    """The best checkpoint is also written after the first epoch: a run of any length leaves one."""
    return (True, 'best') if epoch == 0 or value > best else (False, 'last')


def run_epochs(num_epochs, max_patience, *, rule, train_pass, n_train, val_pass, metric, save, log_path, savepath,
               loadpath, after_train=None, test_pass=None, test_metric=None, reload_best=None, best_name='',
               say=print):
    """The epoch loop.  Per epoch: train_pass() -> the summed cost of n_train steps, read once; after_train();
    val_pass() -> (loss, accuracy, Jaccard counts), metric(counts) -> the value the run stops on; the log line;
    rule(epoch, value, best) -> (improved, tag): improved resets the patience, save(tag, errors) unless tag is None.
    At max_patience or the last epoch: test_pass() (if any) after reload_best() -- False: nothing to reload, the pass
    is skipped --, savepath copied over loadpath if they differ.  Returns the lists (err_train, err_valid, acc_valid,
    jacc_valid)."""
    err_train, err_valid, acc_valid, jacc_valid = [], [], [], []
    patience, best = 0, None
    for epoch in range(num_epochs):
        start_time = time.time()
        err_train.append(float(train_pass()) / n_train)
        if after_train is not None:
            after_train()
        err, acc, jacc_tot = val_pass()
        err_valid.append(err)
        acc_valid.append(acc)
        jacc_valid.append(metric(jacc_tot))                                             # :189-192

        out_str = LOG_LINE % (epoch, err_train[epoch], err_valid[epoch], acc_valid[epoch], jacc_valid[epoch],
                              time.time() - start_time)
        print(out_str)
        with open(log_path, 'a') as f:
            f.write(out_str + '\n')

        improved, tag = rule(epoch, jacc_valid[epoch], best)
        if improved:
            best, patience = jacc_valid[epoch], 0
        else:
            patience += 1
        if tag is not None:
            save(tag, (err_valid, err_train, acc_valid, jacc_valid))                    # :215-217

        if patience == max_patience or epoch == num_epochs - 1:                         # :227-271
            if test_pass is not None and reload_best():
                err, acc, jacc_tot = test_pass()
                print('FINAL MODEL: err test % f, acc test %f, jacc test %f'
                      % (err, acc, (test_metric or metric)(jacc_tot)))
            elif test_pass is not None:
                # (the reference would fail here: it never wrote a best model in a run this short)
                say('no %s was written: the test pass is skipped' % best_name)
            if os.path.abspath(savepath) != os.path.abspath(loadpath):
                say('Copying model and other training files to {}'.format(loadpath))
                shutil.copytree(savepath, loadpath, dirs_exist_ok=True)
            break
    return err_train, err_valid, acc_valid, jacc_valid
