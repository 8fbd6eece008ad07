"""CPU: the fake (meta) implementations of torch.ops.invpref.* as the dispatcher sees them.  An operator whose schema
returns () gets its fake from torch_ops._define; the others compute their output shapes.  No GPU and no library call:
on meta tensors only the fakes run, and an operator without one is an error of the dispatcher ("attempted to run this
operator with Meta tensors") -- under FakeTensorMode alone a missing fake of a () operator would pass unnoticed.
tests/test_torch_ops_gpu.py runs opcheck on the real operators."""
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

from invpref_kdd_2022_amd import torch_ops

VOID = [n for n in torch_ops.NAMES if not getattr(torch.ops.invpref, n).default._schema.returns]


def _argument(arg):
    """a value of the schema argument's type; the shapes do not matter to a fake that returns nothing"""
    t = str(arg.type)
    if t.startswith('Optional['):
        return None
    return {'Tensor': lambda: torch.empty(4, 3, device='meta'), 'List[Tensor]': lambda: [torch.empty(4, 3, device='meta')] * 2,
            'int': lambda: 1, 'float': lambda: 0.5, 'bool': lambda: True, 'List[int]': lambda: [1, 2],
            'List[float]': lambda: [0.5] * 6}[t]()


def test_the_void_operators_are_the_ones_expected():
    assert len(torch_ops.NAMES) == 31 and len(set(torch_ops.NAMES)) == 31
    assert VOID == ['backward', 'train_step_fused', 'train_step_planned_grad_', 'train_step_planned_adam_', 'train_step_alt_',
                    'adam_dense_', 'pack_rows_', 'unpack_rows_', 'adam_ranges_', 'estep_fused_', 'exposure_prior_',
                    'exposure_weights_', 'impute_grad_', 'fairness_grad_', 'cvib_index_', 'cvib_grad_']


@pytest.mark.parametrize('name', VOID)
def test_void_operator_has_a_fake(name):
    op = getattr(torch.ops.invpref, name).default
    args = [_argument(a) for a in op._schema.arguments]
    assert op(*args) is None      # without a registered fake the dispatcher raises here


def test_void_operators_trace_under_fake_tensor_mode():
    with FakeTensorMode():
        P, Q, ws = torch.empty(9, 8), torch.empty(7, 8), torch.empty(64, dtype=torch.uint8)
        sel = torch.empty(4, dtype=torch.int32)
        assert torch.ops.invpref.adam_dense_(P, P.clone(), P.clone(), P.clone(), 1, 0.01, 0.9, 0.999, 1e-8, True) is None
        assert torch.ops.invpref.impute_grad_(P, Q, sel, sel, 0.5, P.clone(), Q.clone(), None, torch.empty(1), ws) is None
        assert torch.ops.invpref.pack_rows_(P, torch.empty(3, dtype=torch.int64), 8, 0, 0, torch.empty(24), True) is None


def test_an_operator_without_a_fake_is_refused_on_meta_tensors():
    """what the test above relies on"""
    lib = torch.library.Library('invpref_test_no_fake', 'DEF')
    lib.define('bare_(Tensor(a!) x) -> ()')
    lib.impl('bare_', lambda x: None, 'CUDA')
    with pytest.raises(NotImplementedError, match='Meta'):
        torch.ops.invpref_test_no_fake.bare_(torch.empty(3, device='meta'))


def test_shape_fakes_still_shape():
    with torch.device('meta'):
        tables = [torch.empty(9, 8), torch.empty(7, 8), torch.empty(9, 8), torch.empty(7, 8), torch.empty(3, 8),
                  torch.empty(3, 8), torch.empty(3)]
        ids = torch.empty(5, dtype=torch.int64)
        inv, env, out = torch.ops.invpref.forward(tables, ids, ids, ids, True)
        assert inv.shape == (5,) and env.shape == (5,) and out.shape == (5, 3) and out.dtype == torch.float32
        items, scores, hits = torch.ops.invpref.predict_topk(tables[0], tables[1], ids, 4, True, None, None, None, None, None,
                                                             None)
        assert items.shape == scores.shape == hits.shape == (5, 4) and items.dtype == torch.int32
        assert torch.ops.invpref.exposure_probability(tables[0], tables[1], None, 6, torch.empty(7), 1.0, 0.1).shape == (6, 7)
