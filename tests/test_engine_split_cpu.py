"""CPU: the seam between the epoch engine (engine.py) and the managers built on it.  The engine's source names nothing of
InvPref's -- no environments, no sample or class weights, no E-step, no cluster events, no alpha schedule -- and never asks
`self._pure` who it is running for; the InvPref and the PureMF managers are siblings under it; a PureMF manager has none of
InvPref's attributes, real or faked.  (The outer loop's return shapes need a device: test_manager_gpu.py.)"""
import inspect
import io
import re
import tokenize

import numpy as np
import torch

from invpref_kdd_2022_amd import baseline as B
from invpref_kdd_2022_amd import synth
from invpref_kdd_2022_amd import train as T
from invpref_kdd_2022_amd.engine import _EpochEngine

# what the engine's body must not name, as whole words (`cluster*`: any identifier that begins so)
FORBIDDEN = ['envs', 'envs_num', '_sample_weights', 'sample_weights', 'class_weights', '_by_env', '_epoch_by_env', '_sw_lazy',
             '_counts_dev', '_es', '_estep_graphs', 'cluster_interval', 'begin_cluster_epoch', 'stop_cluster_epoch',
             'cluster_use_random_sort', 'update_alpha', 'stat_envs']
FORBIDDEN_RE = [r'\b' + re.escape(w) + r'\b' for w in FORBIDDEN] + [r'\bcluster\w*', r'\bmodel\s*\.\s*env_num\b']


def _code_lines(obj) -> list:
    """the source of obj without comments and docstrings, line by line (strings that are statements of their own are
    docstrings; other string literals stay: a name inside getattr(self, '...') is a name)"""
    src = inspect.getsource(obj)
    lines = {}
    prev = None
    for tok in tokenize.generate_tokens(io.StringIO(src).readline):
        if tok.type == tokenize.COMMENT:
            continue
        if tok.type == tokenize.STRING and (prev is None or prev in (tokenize.INDENT, tokenize.NEWLINE, tokenize.NL,
                                                                       tokenize.DEDENT)):
            prev = tok.type
            continue                                            # a docstring
        if tok.type not in (tokenize.NL, tokenize.COMMENT):
            prev = tok.type
        if tok.type in (tokenize.NEWLINE, tokenize.NL, tokenize.INDENT, tokenize.DEDENT, tokenize.ENDMARKER):
            continue
        lines.setdefault(tok.start[0], []).append(tok.string)
    return [' '.join(toks) for _, toks in sorted(lines.items())]


def test_the_stripper_strips_what_it_should():
    class Sample:
        """envs in a docstring"""
        x = 1  # envs in a comment

        def f(self):
            """cluster in a docstring"""
            return getattr(self, 'envs')        # a name in a string literal stays
    code = '\n'.join(_code_lines(Sample))
    assert code.count('envs') == 1 and "'envs'" in code and 'cluster' not in code and 'docstring' not in code


def test_engine_names_nothing_of_invpref():
    code = _code_lines(_EpochEngine)
    assert len(code) > 400                                     # (the engine is all there: the check reads something)
    for pat in FORBIDDEN_RE:
        hits = [ln for ln in code if re.search(pat, ln)]
        assert not hits, (pat, hits[:3])


def test_engine_never_branches_on_pure():
    """`self._pure` only as the `pure=` keyword of an ops call and in the choice of _user_tables: the step's kernel form"""
    for ln in _code_lines(_EpochEngine):
        rest = re.sub(r'pure\s*=\s*self\s*\.\s*_pure\b', '', ln)
        if re.match(r'self\s*\.\s*_user_tables\s*=[^=]', ln):
            continue
        assert not re.search(r'self\s*\.\s*_pure\b', rest), ln
    # and the class attribute bench.py reads is still there, with the managers' two values
    assert T.ImplicitTrainManager._pure is False and B.BasicImplicitTrainManager._pure is True


def test_class_layout():
    assert T._InvPrefTrainManager.__bases__ == (_EpochEngine,) and B._BasicTrainManager.__bases__ == (_EpochEngine,)
    assert not issubclass(B._BasicTrainManager, T._InvPrefTrainManager)
    assert not issubclass(T._InvPrefTrainManager, B._BasicTrainManager)
    for cls in (B.ExpoMFTrainManager, B.WMFTrainManager, B.CVIBTrainManager, B.FairnessMFTrainManager, B.MACRTrainManager,
                B.LinearTransTrainManager, B.CausETrainManager, B.BPRTrainManager, B.IPSBasicTrainManager):
        assert issubclass(cls, B._BasicTrainManager) and not issubclass(cls, T._InvPrefTrainManager)
    # what tests, tools and the benchmark import from train stays importable from there
    for name in ('LOSS_KEYS', 'FlatState', 'RawBatch', 'touched_row_offsets', '_unrank_permutations', '_gc_paused',
                 'transfer_loss_dict_to_line_str', 'ImplicitTrainManager', 'ExplicitTrainManager',
                 'ImplicitTrainStaticPopularityManager', '_InvPrefTrainManager'):
        assert hasattr(T, name), name


class _Stub:
    def evaluate(self):
        return {}


def test_a_pure_mf_manager_has_nothing_of_invpref():
    U, I, D, n, bs = 40, 30, 16, 300, 128                      # (test_lazy_adam_cpu.py's shape)
    data = torch.from_numpy(synth.interactions(1, U, I, n))
    mgr = B.BasicImplicitTrainManager(B.PureMatrixFactorization(U, I, D), _Stub(), torch.device('cpu'), data, bs, 3, 10 ** 9,
                                      0.01, 0., 0.)
    for name in ('envs', 'class_weights', 'cluster', 'stat_envs', 'cluster_a_batch', 'update_each_env_count',
                 'cluster_interval', 'update_alpha'):
        assert not hasattr(mgr, name), name
    # the engine's defaults are PureMF's answers
    assert mgr._batch_inputs(0, 5) == (None, None) and mgr._resident() == () and mgr._graph_key_extra() is None
    assert mgr._alpha_for(0) == 0. and not mgr._alpha_scheduled() and mgr._env_count == 0
    assert not any(mgr._ends_run(e) for e in range(1, 200))
    w = torch.arange(3.)
    assert mgr._step_weights(w) == (w, mgr._flags)
    # one run of epochs up to the end of training or the 64-epoch bound, no event of its own in between
    mgr.epochs = 1000
    assert mgr._epochs_to_next_event() == 64
    mgr.epochs, mgr.evaluate_interval = 10, 4
    assert mgr._epochs_to_next_event() == 4
    assert np.isfinite(mgr._coefs(0.)).all()
