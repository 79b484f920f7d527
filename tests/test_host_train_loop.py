"""CPU (no launch, no device): the epoch loop both training drivers run (train_loop.run_epochs)
on fake passes that return scripted validation values and fake save actions that record (epoch, tag) -- the two
best / last / patience rules against hand-worked sequences and against a literal restatement of the loops the drivers
had before they shared one --, and the chunks train._NetTrainer cuts a net's weight ranges into."""
import math
import os
import random
import re
import subprocess
import sys

import pytest

LOG = 'EPOCH %i: Avg epoch training cost train %f, cost val %f, acc val %f, jacc val %f took '
NAN = float('nan')
VALUES = [0.3, 0.5, 0.4, 0.6, 0.6, 0.2, 0.9, 0.9]
BEST = 'new_fcn8_model_best.npz'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Run:
    """One run of run_epochs on fakes: `events` in order, `saves` one entry per epoch run (None: nothing written),
    `said` the messages, `lists` the result."""

    def __init__(self, rule, values, folder, max_patience=2, num_epochs=None, loadpath=None, test=True, hook=True):
        from iterative_inference_segm_amd import train_loop
        self.events, self.said, self.epoch = [], [], -1
        values = list(values)
        savepath = os.path.join(str(folder), 'save')
        os.makedirs(savepath, exist_ok=True)
        self.log = os.path.join(savepath, 'output.log')
        self.loadpath = savepath if loadpath is None else os.path.join(str(folder), loadpath)

        def train_pass():
            self.epoch += 1
            self.events.append('train')
            return 6.0 + self.epoch                      # the summed cost of three steps

        def val_pass():
            self.events.append('val')
            return 0.25 * self.epoch, 0.5, values[self.epoch]

        def reload_best():
            self.events.append('reload')
            return ('save', 'best') in [(e[0], e[2]) for e in self.events if isinstance(e, tuple)]

        self.lists = train_loop.run_epochs(
            len(values) if num_epochs is None else num_epochs, max_patience, rule=rule, train_pass=train_pass,
            n_train=3, val_pass=val_pass, metric=float, log_path=self.log,
            save=lambda tag, errors: self.events.append(('save', len(errors[0]) - 1, tag)),
            after_train=(lambda: self.events.append('hook')) if hook else None,
            test_pass=(lambda: self.events.append('test') or (0.5, 0.5, 0.75)) if test else None,
            reload_best=reload_best, best_name=BEST, savepath=savepath, loadpath=self.loadpath, say=self.said.append)
        by_epoch = {e[1]: e[2] for e in self.events if isinstance(e, tuple)}
        self.saves = [by_epoch.get(i) for i in range(self.epoch + 1)]


def _rules():
    from iterative_inference_segm_amd import train_loop
    return {'fcn8': train_loop.fcn8_rule, 'densenet': train_loop.first_epoch_best_rule}


@pytest.mark.parametrize('net,want', [('fcn8', [None, 'last', 'best', 'best', 'last', 'last']),
                                      ('densenet', ['best', 'best', 'last', 'best', 'last', 'last'])])
def test_the_hand_worked_sequence(tmp_path, net, want):
    r = Run(_rules()[net], VALUES, tmp_path, max_patience=2, num_epochs=8)
    assert r.saves == want and r.epoch == 5                              # stops after epoch 5
    assert [len(v) for v in r.lists] == [6] * 4
    err_train, err_valid, acc_valid, jacc_valid = r.lists
    assert err_train == [(6.0 + e) / 3 for e in range(6)] and err_valid == [0.25 * e for e in range(6)]
    assert acc_valid == [0.5] * 6 and jacc_valid == VALUES[:6]
    # the test pass: once, at the stop, on the reloaded best weights
    assert r.events[-2:] == ['reload', 'test'] and r.events.count('test') == 1 and r.events.count('reload') == 1


@pytest.mark.parametrize('net,want', [('fcn8', [None, 'last', 'best', 'last', 'best']),
                                      ('densenet', ['best', 'last', 'best', 'last', 'best'])])
def test_a_nan_is_never_the_best_and_costs_one_patience(tmp_path, net, want):
    # were the NaN taken as the best value, 0.6 > nan would be False and the last epoch a 'last'; were it free, the
    # run under max_patience=1 below would go on
    assert Run(_rules()[net], [0.3, 0.2, 0.5, NAN, 0.6], tmp_path, max_patience=3).saves == want
    r = Run(_rules()[net], [0.3, 0.2, 0.5, NAN, 0.6], tmp_path / 'b', max_patience=1)
    assert r.epoch == 1 and r.saves == want[:2]
    r = Run(_rules()[net], [0.3, 0.4, 0.5, NAN, 0.6], tmp_path / 'c', max_patience=1)
    assert r.epoch == (1 if net == 'fcn8' else 3) and r.saves[-1] == 'last'


def test_two_epochs_under_the_fcn8_rule_write_no_best_and_skip_the_test_pass(tmp_path, capsys):
    r = Run(_rules()['fcn8'], [0.3, 0.9], tmp_path, num_epochs=2)
    assert r.saves == [None, 'last']
    assert 'test' not in r.events and r.events[-1] == 'reload'
    assert r.said == ['no %s was written: the test pass is skipped' % BEST]
    assert 'FINAL MODEL' not in capsys.readouterr().out
    # the other rule always has one; and no test split, no reload
    r = Run(_rules()['densenet'], [0.3, 0.9], tmp_path / 'b', num_epochs=2)
    assert r.saves == ['best', 'best'] and r.events[-2:] == ['reload', 'test'] and r.said == []
    assert 'FINAL MODEL: err test  0.500000, acc test 0.500000, jacc test 0.750000' in capsys.readouterr().out
    r = Run(_rules()['densenet'], [0.3, 0.9], tmp_path / 'c', num_epochs=2, test=False)
    assert 'reload' not in r.events and 'test' not in r.events and r.said == []


@pytest.mark.parametrize('net', ['fcn8', 'densenet'])
def test_the_last_epoch_stops_the_run_with_patience_left(tmp_path, net):
    r = Run(_rules()[net], [0.1, 0.2, 0.3, 0.4], tmp_path, max_patience=2, num_epochs=3)
    assert r.epoch == 2 and r.saves[-1] == 'best' and r.events[-1] == 'test'
    assert Run(_rules()[net], [0.5], tmp_path / 'b', max_patience=1).saves == [None if net == 'fcn8' else 'best']


def test_the_hook_runs_once_per_epoch_between_the_train_and_the_validation_pass(tmp_path):
    r = Run(_rules()['densenet'], VALUES, tmp_path, max_patience=2)
    per_epoch = [e for e in r.events if not isinstance(e, tuple)][:-2]
    assert per_epoch == ['train', 'hook', 'val'] * 6
    assert 'hook' not in Run(_rules()['fcn8'], VALUES, tmp_path / 'b', hook=False).events


def test_one_log_line_per_epoch_on_stdout_and_in_the_file(tmp_path, capsys):
    r = Run(_rules()['densenet'], VALUES, tmp_path, max_patience=2)
    out = [l for l in capsys.readouterr().out.splitlines() if l.startswith('EPOCH')]
    lines = open(r.log).read().splitlines()
    assert lines == out and len(lines) == 6
    for e, line in enumerate(lines):
        head = LOG % (e, (6.0 + e) / 3, 0.25 * e, 0.5, VALUES[e])
        assert line.startswith(head) and re.fullmatch(r'\d+\.\d{6} s', line[len(head):]), line


def test_copytree_only_when_the_two_folders_differ(tmp_path):
    r = Run(_rules()['densenet'], [0.3, 0.2], tmp_path / 'same')
    assert r.said == [] and os.listdir(str(tmp_path / 'same')) == ['save']
    r = Run(_rules()['densenet'], [0.3, 0.2], tmp_path / 'apart', loadpath='load')
    assert r.said == ['Copying model and other training files to ' + r.loadpath]
    assert open(os.path.join(r.loadpath, 'output.log')).read() == open(r.log).read()


def test_importing_the_module_and_parsing_arguments_load_no_torch():
    """In a fresh process: the import, both drivers' parsers and a refusal leave torch unloaded."""
    code = ('import sys; sys.path.insert(0, %r)\n'
            'import iterative_inference_segm_amd.train_loop as L\n'
            'assert "torch" not in sys.modules, "import"\n'
            'import train_fcn8, train_fcdensenet\n'
            'train_fcn8.parse_args(["--kxk", "bf16"]); train_fcdensenet.parse_args(["--deconv", "bf16"])\n'
            'L.check_switches("float32", wgrad="bf16")\n'
            'assert L.main("x.py", lambda: L.check_switches("float64", wgrad="bf16"), None) == 2\n'
            'assert "torch" not in sys.modules, "parsers and refusals"\n' % ROOT)
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stderr.startswith("x.py: wgrad='bf16'")


# ---- the loops the two drivers had, restated line for line, against the rules ----
def _parent_fcn8(values, max_patience):
    saves, patience, best = [], 0, None
    for epoch, v in enumerate(values):
        if epoch == 0:
            best = v
            saves.append(None)
        elif epoch > 1 and v > best:
            best, patience = v, 0
            saves.append('best')
        else:
            patience += 1
            saves.append('last')
        if patience == max_patience or epoch == len(values) - 1:
            return saves


def _parent_densenet(values, max_patience):
    saves, patience, best = [], 0, None
    for epoch, v in enumerate(values):
        if epoch == 0 or v > best:
            best, patience = v, 0
            saves.append('best')
        else:
            patience += 1
            saves.append('last')
        if patience == max_patience or epoch == len(values) - 1:
            return saves


def test_the_rules_are_the_drivers_former_loops_on_random_sequences(tmp_path):
    rng = random.Random(7)
    ties = nans = 0
    for i in range(300):
        values = []
        for _ in range(rng.randint(1, 12)):
            u = rng.random()
            if values and u < 1 / 3:
                values.append(rng.choice(values))                        # a tie with an earlier value
                ties += 1
            elif u < 0.4:
                values.append(NAN)
                nans += 1
            else:
                values.append(round(rng.random(), 2))
        patience = rng.randint(1, 4)
        for net, parent in (('fcn8', _parent_fcn8), ('densenet', _parent_densenet)):
            r = Run(_rules()[net], values, tmp_path / ('%s%d' % (net, i)), max_patience=patience, test=False)
            assert r.saves == parent(values, patience), (net, values, patience)
    assert ties > 400 and nans > 60
    assert math.isnan(NAN) and not NAN > 0.5 and not 0.5 > NAN           # what both rules lean on


# ---- the trainer's chunks ----
@pytest.mark.parametrize('n,chunks', [(0, 0), (1, 1), (64, 1), (65, 2), (200, 4)])
def test_net_trainer_cuts_the_weight_ranges_into_chunks_the_l2_kernel_takes(n, chunks):
    import torch
    from iterative_inference_segm_amd import _lib
    from iterative_inference_segm_amd.train import DenseNetTrainer, FCN8Trainer
    assert _lib.L2_MAX_RANGES == 64

    class Net:
        trainable, flat = True, torch.zeros(3 * n + 1)

        def weight_ranges(self):
            return [(3 * i, 3 * i + 2) for i in range(n)]

    for cls in (FCN8Trainer, DenseNetTrainer):
        got = cls(Net(), 4, [4], weight_decay=1e-4).ranges
        assert len(got) == chunks and all(1 <= len(c) <= 64 for c in got)
        assert [len(c) for c in got[:-1]] == [64] * (chunks - 1 if chunks else 0)
        assert [r for c in got for r in c] == Net().weight_ranges()      # in order, every range once
        with pytest.raises(ValueError, match='weight_decay must be >= 0'):
            cls(Net(), 4, [4], weight_decay=-1e-4)
