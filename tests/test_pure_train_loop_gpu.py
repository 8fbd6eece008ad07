"""GPU: train() of the PureMF managers with per-epoch read-backs and printed lines (silent=False) against the deferred form
(silent=True): the same records, bit for bit, and the printed lines in the reference loop's order.  Beside
test_expomf_gpu.py::test_train_verbose_path_matches, for the managers whose runs span several epochs."""
import numpy as np
import pytest
import torch

from invpref_kdd_2022_amd.baseline import (BasicExplicitTrainManager, BasicImplicitTrainManager,
                                           PureExplicitMatrixFactorization, PureMatrixFactorization, WMFTrainManager,
                                           wmf_distinct, wmf_draw_epochs)

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
U, I, D, N, BS, EPOCHS = 40, 30, 8, 200, 64, 5      # four minibatches, the last one ragged (8 rows)


class Stub:
    batch_size = 96

    def evaluate(self):
        return {}


def _inputs(implicit: bool):
    rs = np.random.RandomState(2024)
    y = rs.randint(0, 2, N) if implicit else rs.randint(1, 6, N)
    data = np.stack([rs.randint(0, U, N), rs.randint(0, I, N), y], axis=1).astype(np.int64)
    init = {'user_emb.weight': (rs.standard_normal((U, D)) * 0.1).astype(np.float32),
            'item_emb.weight': (rs.standard_normal((I, D)) * 0.1).astype(np.float32)}
    return data, init


@pytest.mark.parametrize('cls', [BasicImplicitTrainManager, BasicExplicitTrainManager, WMFTrainManager],
                         ids=lambda c: c.__name__)
def test_train_verbose_path_matches(cls, capsys):
    """5 epochs, evaluations at epochs 0, 2 and 4: the runs are cut after epochs 2 and 4 and one epoch is left at the end"""
    data, init = _inputs(cls.implicit)
    kw = {}
    if cls is WMFTrainManager:      # both runs see the same recorded draws
        state = np.random.get_state()
        np.random.seed(7)
        recorded = wmf_draw_epochs(wmf_distinct(data[:, 0], data[:, 1], BS), 16, 12, EPOCHS)
        np.random.set_state(state)
        kw = dict(imputation_coe=0.5, user_batch_size=16, item_batch_size=12)

    def run(silent):
        model = (PureMatrixFactorization if cls.implicit else PureExplicitMatrixFactorization)(U, I, D)
        model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in init.items()})
        if cls is WMFTrainManager:
            kw['selections'] = list(recorded)
        mgr = cls(model, Stub(), DEV, torch.from_numpy(data), BS, EPOCHS, 2, 0.01, 0.05, 0.01, 2, **kw)
        assert mgr.batch_num == 4
        capsys.readouterr()
        out = mgr.train(silent=silent)
        assert len(out) == 2
        return out, capsys.readouterr().out

    ((la, ea), (ta, tea)), quiet = run(True)
    ((lb, eb), (tb, teb)), loud = run(False)
    assert ea == eb == [1, 2, 3, 4, 5] and tea == teb == [0, 2, 4]
    assert ta == tb == [{}, {}, {}]
    assert all(np.isfinite(list(d.values())).all() for d in la)
    assert la == lb                                             # floats compared exactly
    marks = [ln for ln in loud.splitlines() if ln.startswith(('test at epoch:', 'train epoch:'))]
    assert marks == ['test at epoch: 0', 'train epoch: 1', 'train epoch: 2', 'test at epoch: 2', 'train epoch: 3',
                     'train epoch: 4', 'test at epoch: 4', 'train epoch: 5']
    assert not [ln for ln in quiet.splitlines() if ln.startswith(('test at epoch:', 'train epoch:'))]
    # every marker is followed by its record's line
    lines = loud.splitlines()
    at = [i for i, ln in enumerate(lines) if ln.startswith('train epoch:')]
    assert [lines[i + 1] for i in at] == [', '.join(f'{k}: {v}' for k, v in d.items()) for d in lb]
