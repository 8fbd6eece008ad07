"""GPU: the device-side Adam schedule (include/invpref_hip.h: InvPrefAdamSchedule) that every optimiser step reads its
per-step scalars from under HIP-graph replay -- step_size, bc2_sqrt, a scheduled gradient-reversal alpha and, for the
alternating form, the fold-flag generation and the previous step's two scalars in state words 10 / 11.

Operator level: the same k steps once with sched=None and explicit step numbers, once per scenario with
sched=(state, table, step & 1) -- for each of the four kernels that move the schedule on (mstep_apply_kernel, its wide copy
with the D = 256 classifier, mstep_alt_kernel, adam_ranges_kernel behind a gradient pass that only reads the slot).  Both
runs go through the same kernel instance and launch geometry, and invpref_adam_schedule_fill computes the same floats as
the eager entry points: parameters, both moments and the six loss terms of every step agree BITWISE; after every launch
the 32 state words are read back and compared with what the header says they hold.

Manager level: one training twice with identical calls, once with the shipped table of 8192 rows (no refill at this
length) and once with a small table (_SCHED_N patched): both capture and replay the same graphs and differ only in where
the table ends, so every loss, parameter and moment agrees bitwise."""
import functools

import numpy as np
import pytest
import torch

from invpref_kdd_2022_amd import _capi, ops, plan as planlib, synth
from invpref_kdd_2022_amd.baseline import BasicImplicitTrainManager, PureMatrixFactorization
from invpref_kdd_2022_amd.models import InvPrefExplicit, InvPrefImplicit
from invpref_kdd_2022_amd.engine import _EpochEngine
from invpref_kdd_2022_amd.train import LOSS_KEYS, ExplicitTrainManager, ImplicitTrainManager

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
COEFS = (2.05, 8.63, 5.1, 7.73, 0.0015, 1.74)
PURE_COEFS = (1., 0., 0., 0.6, 0.1, 0.)
FIRST, LR, K = 5, 0.01, 7
POISON = 0x5A5AA5A5                                   # what the test leaves in state words nobody has written yet
STEP_ALPHAS = tuple(0.3 + 0.17 * c for c in range(K))   # scenario (d): a per-step alpha in column 6
CALL_ALPHA = 123.0                                    # ... and a deliberately different one in the call's coefficients


# ------------------------------------------------------------------------------------------ the schedule, as a caller keeps it
def _fill(first_step: int, n: int) -> np.ndarray:
    host = np.zeros((n, 8), np.float32)
    _capi.check(_capi.lib().invpref_adam_schedule_fill(host.ctypes.data, first_step, n, LR, 0.9, 0.999, 1e-8),
                'invpref_adam_schedule_fill')
    return host


class Schedule:
    """table: device float32 [n, 8], row j for step base + j; state: device int32 [32], two slots of 16 words"""

    def __init__(self, n: int, base: int, alphas=None):
        self.n, self.alphas = n, alphas
        self.table = torch.zeros(n, 8, dtype=torch.float32, device=DEV)
        self.state = torch.zeros(32, dtype=torch.int32, device=DEV)
        self.refill(base)

    def refill(self, base: int):
        host = _fill(base, self.n)
        assert np.isnan(host[:, 6]).all()                # as the fill leaves it: "the alpha of the call's coefficient block"
        if self.alphas is not None:
            for j in range(self.n):
                if 0 <= base + j - FIRST < K:
                    host[j, 6] = np.float32(self.alphas[base + j - FIRST])
        self.table.copy_(torch.from_numpy(host))
        self.base, self.host = base, host

    def row_bits(self, step: int) -> np.ndarray:
        return self.host[step - self.base].view(np.int32)

    def write_slot(self, step: int, prev_scalars=None):
        """slot step & 1 = {step, base, row} for the step about to run, every other word zero (the alternating form in the
        middle of a run: words 10 / 11 = the previous step's step_size / bc2_sqrt); the other slot: a bit pattern"""
        st, o = np.zeros(32, np.int32), 16 * (step & 1)
        st[o], st[o + 1] = step, self.base
        st[o + 2:o + 10] = self.row_bits(step)
        if prev_scalars is not None:
            st[o + 10:o + 12] = prev_scalars
        st[16 - o:32 - o] = POISON
        self.state.copy_(torch.from_numpy(st))

    def poison_other(self, step: int):
        """nobody reads the other slot before the launch of `step` has filled it: whatever it leaves alone stays visible"""
        o = 16 * ((step & 1) ^ 1)
        self.state[o:o + 16] = POISON

    def read(self) -> np.ndarray:
        return self.state.cpu().numpy()       # (a host sync per launch: fine in a test)


class Run:
    """One pass over the K steps: eager (rows == 0: explicit step numbers, the step's alpha in the coefficient block) or
    through a schedule of `rows` rows whose row 0 belongs to step `base`; `alphas`: scenario (d)."""

    def __init__(self, rows: int = 0, base: int = FIRST, alphas=None, alt: bool = False):
        self.alphas, self.alt, self.refills, self.ends_seen = alphas, alt, 0, 0
        self.sc = Schedule(rows, base, alphas) if rows else None

    def begin(self, c: int):
        sc, step = self.sc, FIRST + c
        if sc is None:
            return
        if c == 0:
            sc.write_slot(step)
        elif step - sc.base >= sc.n:
            # the table ended with the previous step: refill with base = this step and rewrite the slot, as a caller must
            prev = sc.row_bits(step - 1)[:2].copy() if self.alt else None
            sc.refill(step)
            sc.write_slot(step, prev)
            self.refills += 1
        sc.poison_other(step)
        self.before = sc.read()

    def kw(self, c: int) -> dict:
        if self.sc is None:
            return dict(step=FIRST + c, lr=LR, sched=None)
        return dict(step=0, lr=0.0, sched=(self.sc.state, self.sc.table, (FIRST + c) & 1))   # (step / lr: not looked at)

    def coefs(self, c: int, coefs):
        if self.alphas is None:
            return coefs
        return tuple(coefs[:5]) + ((self.alphas[c],) if self.sc is None else (CALL_ALPHA,))

    def advanced(self, c: int):
        """after the launch that ends step FIRST + c: the other slot holds the next step, the consumed one is as it was"""
        sc, step = self.sc, FIRST + c
        if sc is None:
            return
        got, want = sc.read(), self.before.copy()
        cur, nxt = 16 * (step & 1), 16 * ((step & 1) ^ 1)
        np.testing.assert_array_equal(got[cur:cur + 16], self.before[cur:cur + 16])      # the slot just consumed
        assert (got[nxt], got[nxt + 1]) == (step + 1, sc.base)
        want[nxt], want[nxt + 1] = step + 1, sc.base
        if step + 1 - sc.base < sc.n:
            want[nxt + 2:nxt + 10] = sc.row_bits(step + 1)
        else:       # the successor's row lies beyond the table: its scalars are left alone
            self.ends_seen += 1
            assert (got[nxt + 2:nxt + 10] == np.int32(POISON)).all()
        if self.alt:
            want[nxt + 10:nxt + 12] = sc.row_bits(step)[:2]
        np.testing.assert_array_equal(got, want)     # (words 12..15, and 10 / 11 of the two-launch forms: still the pattern)
        self.before = got

    def unchanged(self):
        """after a launch that only reads the slot (a gradient pass, the alternating form's flush)"""
        if self.sc is not None:
            np.testing.assert_array_equal(self.sc.read(), self.before)


# ------------------------------------------------------------------------------------------ the step forms
SIZES = (700,) * 6 + (333,)
SIZES_256 = (500,) * 6 + (77,)
#        kind,  U,   I,  E,  D,   minibatch sizes, PureMF, lanes per group
FORMS = {
    'fused_16_lanes': ('rows', 300, 40, 4, 64, SIZES, False, 16),
    'fused_16_lanes_pure_mf': ('rows', 400, 90, 1, 20, SIZES, True, 16),
    'wide_rows_d128': ('rows', 60, 9, 8, 128, SIZES, False, 16),
    'mfma_classifier_d256': ('rows', 40, 12, 16, 256, SIZES_256, False, 32),
    'alternating': ('alt', 300, 40, 4, 64, SIZES, False, 16),
    'alternating_pure_mf': ('alt', 300, 40, 1, 64, SIZES, True, 16),
    'grad_then_ranged_adam_d64': ('grad', 300, 40, 4, 64, SIZES, False, 16),
    'grad_then_ranged_adam_d256': ('grad', 40, 12, 16, 256, SIZES_256, False, 32),
}


@functools.lru_cache(maxsize=None)
def _inputs(form: str):
    """data, plans and the initial state of a form: built once, never written to (every run works on clones)"""
    kind, U, I, E, D, sizes, pure, lanes = FORMS[form]
    seed, N = 11 + U + D, int(sum(sizes))
    assert len(sizes) == K
    rs = np.random.RandomState(seed)
    data = synth.interactions(seed, U, I, N, implicit=True)
    offs = np.concatenate([[0], np.cumsum(sizes)])
    y = torch.from_numpy(data[:, 2].astype(np.float32)).to(DEV)
    e = None if pure else torch.from_numpy(rs.randint(0, E, N).astype(np.int64)).to(DEV)
    w = None if pure else torch.from_numpy(rs.uniform(0.1, 1, N).astype(np.float32)).to(DEV)
    coefs = PURE_COEFS if pure else COEFS
    flags = (ops.flags_of(True, False, False, True, False, dense_reg=False) if pure
             else ops.flags_of(True, True, True, False, True))
    # non-zero moments (tests/test_alt_gpu.py::_state): with zero moments the first update is lr * g / (|g| + eps)
    tabs = synth.tables(seed, U, I, E, D, std=0.2)
    names = ops.PARAM_NAMES[:2] if pure else ops.PARAM_NAMES
    rs2 = np.random.RandomState(seed + 1)
    P = [torch.from_numpy(np.ascontiguousarray(tabs[k], np.float32)).to(DEV) for k in names]
    M = [torch.from_numpy((1e-3 * rs2.standard_normal(p.shape)).astype(np.float32)).to(DEV) for p in P]
    V = [torch.from_numpy((1e-5 * rs2.random_sample(p.shape) + 1e-8).astype(np.float32)).to(DEV) for p in P]

    def mb(c):
        s = slice(int(offs[c]), int(offs[c + 1]))
        return data[s, 0], data[s, 1], data[s, 2].astype(np.float32)

    if kind == 'alt':
        assert ops.alt_supported(P)
        apl = []
        for c in range(K):
            apl.append(planlib.build_alt_plan(mb(c), None if c == 0 else mb(c - 1)[:2], c % 2, U, I, factor_num=D,
                                              n_partials_prev=apl[-1]['n_tasks'] if c else 0))
        apl.append(planlib.build_alt_plan(None, mb(K - 1)[:2], K % 2, U, I, factor_num=D, n_partials_prev=apl[-1]['n_tasks']))
        plans = [planlib.upload_alt(p, DEV) for p in apl]
        extra = max(p['n_tasks'] for p in apl) + 1
    else:
        host_plans = [planlib.build_row_plan(*mb(c), U, I, factor_num=D, env_num=E) for c in range(K)]
        assert all(p['lanes_per_group'] == lanes for p in host_plans)     # 16 lanes up to 128 floats a row, 32 beyond
        assert ops.alt_supported(P) == (D <= 64 and E <= 4)
        plans = [planlib.upload(p, DEV) for p in host_plans]
        extra = None
    return dict(kind=kind, sizes=sizes, pure=pure, offs=offs, y=y, e=e, w=w, coefs=coefs, flags=flags, state=(P, M, V),
                plans=plans, extra=extra)


def _sl(t, offs, c):
    return None if t is None else t[int(offs[c]):int(offs[c + 1])]


def _run_rows(x, run: Run):
    """two launches per step, parameters ping-pong (ops.mstep_rows_adam): the 16-lane, wide and 256-float instances"""
    P, M, V = ([t.clone() for t in part] for part in x['state'])
    a, b = P, [p.clone() for p in P]
    ws, losses, offs, sizes = ops.Workspace(DEV), torch.zeros(K, 6, device=DEV), x['offs'], x['sizes']
    for c in range(K):
        run.begin(c)
        kw = run.kw(c)
        ops.mstep_rows_adam(a, b, M, V, x['plans'][c], _sl(x['e'], offs, c), _sl(x['y'], offs, c), _sl(x['w'], offs, c),
                            sizes[c], run.coefs(c, x['coefs']), x['flags'], losses[c], kw['step'], kw['lr'], ws,
                            pure=x['pure'], sched=kw['sched'])
        run.advanced(c)
        a, b = b, a
    return [t.cpu().numpy() for t in a + M + V] + [losses.cpu().numpy()]


def _run_alt(x, run: Run):
    """one alternating launch per step + the flush (ops.mstep_alt), as tests/test_alt_gpu.py::run_both issues them"""
    P, M, V = ([t.clone() for t in part] for part in x['state'])
    offs, sizes, pure = x['offs'], x['sizes'], x['pure']
    aws = ops.AltWorkspace(P, max(sizes), x['extra'], pure=pure)
    losses = torch.zeros(K, 6, device=DEV)
    for c in range(K):
        run.begin(c)
        kw = run.kw(c)
        ops.mstep_alt(P, M, V, x['plans'][c], _sl(x['e'], offs, c), _sl(x['w'], offs, c), sizes[c],
                      sizes[c - 1] if c else sizes[c], run.coefs(c, x['coefs']), x['flags'], losses[c - 1] if c else None,
                      kw['step'], kw['lr'], aws, c & 1, pure=pure, sched=kw['sched'])
        run.advanced(c)
    kw = run.kw(K - 1)                            # the flush runs in the LAST step's slot and leaves the schedule alone
    ops.mstep_alt(P, M, V, x['plans'][K], None, None, sizes[K - 1], sizes[K - 1], run.coefs(K - 1, x['coefs']), x['flags'],
                  losses[K - 1], kw['step'], kw['lr'], aws, K & 1, pure=pure, sched=kw['sched'])
    run.unchanged()
    torch.cuda.synchronize()
    assert aws.error() == 0
    return [t.cpu().numpy() for t in P + M + V] + [losses.cpu().numpy()]


def _run_grad(x, run: Run):
    """gradient pass (reads the slot) + ranged Adam (moves the schedule on) over tables that are views of one flat buffer,
    in three pieces -- the sequence of a sharded rank and of INVPREF_UNFUSED=1"""
    shapes = [tuple(t.shape) for t in x['state'][0]]
    counts = [int(np.prod(s)) for s in shapes]
    n = sum(counts)
    assert all(k % 4 == 0 for k in counts)
    flat = [torch.cat([t.reshape(-1) for t in part]) for part in x['state']] + [torch.zeros(n, device=DEV)]
    fp, fm, fv, fg = flat
    assert all(t.data_ptr() % 16 == 0 for t in flat)
    at = np.concatenate([[0], np.cumsum(counts)])
    Pv, Gv = ([t[int(at[i]):int(at[i + 1])].view(s) for i, s in enumerate(shapes)] for t in (fp, fg))
    cut1, cut2 = n // 3 // 4 * 4, 2 * n // 3 // 4 * 4                 # three pieces, cut inside tables
    offsets, lengths = [0, cut1, cut2], [cut1, cut2 - cut1, n - cut2]
    ws, losses, offs, sizes = ops.Workspace(DEV), torch.zeros(K, 6, device=DEV), x['offs'], x['sizes']
    for c in range(K):
        run.begin(c)
        kw = run.kw(c)
        ops.mstep_rows_grad(Pv, Gv, x['plans'][c], _sl(x['e'], offs, c), _sl(x['y'], offs, c), _sl(x['w'], offs, c),
                            sizes[c], run.coefs(c, x['coefs']), x['flags'], losses[c], ws, sched=kw['sched'])
        run.unchanged()
        # (the planned gradient pass overwrites every row: nothing to zero, as in the managers' sequence)
        ops.adam_ranges_(fp, fg, fm, fv, offsets, lengths, kw['step'], kw['lr'], zero_grad=False, sched=kw['sched'])
        run.advanced(c)
    return [t.cpu().numpy() for t in (fp, fm, fv, fg)] + [losses.cpu().numpy()]


_RUNNERS = dict(rows=_run_rows, alt=_run_alt, grad=_run_grad)


def _go(form: str, run: Run):
    x = _inputs(form)
    out = _RUNNERS[x['kind']](x, run)
    assert all(np.isfinite(a).all() for a in out)
    return out


@functools.lru_cache(maxsize=None)
def _eager(form: str, with_alphas: bool = False):
    """the reference of every scenario: computed once per form, shared, never modified"""
    return _go(form, Run(alphas=STEP_ALPHAS if with_alphas else None, alt=FORMS[form][0] == 'alt'))


@functools.lru_cache(maxsize=None)
def _scenario_a(form: str):
    run = Run(rows=16, base=FIRST, alt=FORMS[form][0] == 'alt')
    out = _go(form, run)
    assert run.refills == 0 and run.ends_seen == 0
    return out


def _same(got, want):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(a, b, err_msg=f'array {i} (parameters, exp_avg, exp_avg_sq ..., losses last)')


@pytest.mark.parametrize('form', list(FORMS))
def test_a_table_based_at_the_first_step(form):
    # (column 6 holds the fill's NaN: the alpha of the call's coefficient block is the one used -- scenario (d), first half)
    _same(_scenario_a(form), _eager(form))


@pytest.mark.parametrize('form', list(FORMS))
def test_b_table_based_before_the_first_step(form):
    run = Run(rows=16, base=FIRST - 3, alt=FORMS[form][0] == 'alt')      # the first row used is row 3
    _same(_go(form, run), _eager(form))
    assert run.refills == 0 and run.ends_seen == 0


@pytest.mark.parametrize('form', list(FORMS))
def test_c_table_ends_in_the_middle_of_the_run(form):
    """4 rows for 7 steps: the launch of step FIRST + 3 finds its successor's row beyond the table and leaves that slot's
    scalars alone (Run.advanced asserts the pattern is still there; the alternating form writes words 10 / 11 all the
    same); the caller refills with base = FIRST + 4, rewrites the slot and goes on -- to the same result."""
    run = Run(rows=4, base=FIRST, alt=FORMS[form][0] == 'alt')
    got = _go(form, run)
    assert run.refills == 1 and run.ends_seen == 1
    _same(got, _scenario_a(form))
    _same(got, _eager(form))


@pytest.mark.parametrize('form', [f for f in FORMS if not FORMS[f][6]])
def test_d_alpha_from_column_6(form):
    """a per-step alpha in column 6 wins over the call's coefficient block (which holds 123.0 here): the result is the eager
    run given that step's alpha in its coefficients -- and not the run with the coefficient block's own alpha"""
    run = Run(rows=16, base=FIRST, alphas=STEP_ALPHAS, alt=FORMS[form][0] == 'alt')
    _same(_go(form, run), _eager(form, True))
    assert not np.array_equal(_eager(form, True)[-1], _eager(form)[-1])      # (alpha does move the loss terms)


# ------------------------------------------------------------------------------------------ refills through the managers
class _Stub:
    batch_size = 96

    def evaluate(self):
        return {'stub': 0.0}


_Y = dict(U=300, I=40, E=4, D=64, n=2000, bs=700)
_W = dict(U=300, I=200, E=5, D=256, n=2500, bs=1024)
MANAGERS = {
    'implicit_alternating': dict(_Y, cls=ImplicitTrainManager, alt=True),
    'implicit_two_launch': dict(_Y, cls=ImplicitTrainManager, env={'INVPREF_ALT': '0'}, alt=False),
    'explicit': dict(_Y, cls=ExplicitTrainManager),
    'wide_rows_e8_d128': dict(U=60, I=9, E=8, D=128, n=2000, bs=700, cls=ImplicitTrainManager, alt=False),
    'd256_fused': dict(_W, cls=ImplicitTrainManager, alt=False),
    'd256_gradient_pass_and_ranged_adam': dict(_W, cls=ImplicitTrainManager, env={'INVPREF_UNFUSED': '1'}, alt=False),
    'implicit_alternating_alpha_schedule': dict(_Y, cls=ImplicitTrainManager, alpha=None, alt=True),
    'd256_gradient_pass_alpha_schedule': dict(_W, cls=ImplicitTrainManager, env={'INVPREF_UNFUSED': '1'}, alpha=None, alt=False),
    'pure_mf': dict(U=400, I=90, E=1, D=20, n=2000, bs=700, cls=BasicImplicitTrainManager),
}
_SWITCHES = ('INVPREF_ALT', 'INVPREF_UNFUSED', 'INVPREF_NO_GRAPH', 'INVPREF_NO_PLAN', 'INVPREF_FORCE_SHARDED_PATH',
             'INVPREF_ALT_MAX_CHAIN', 'INVPREF_WEIGHTS_BY_ENV')


def _train(name: str, sched_n: int, monkeypatch, no_graph: bool = False) -> dict:
    """one training: batch_num = 3 with a ragged last minibatch; runs of 1, 8, 8, 1, 5, 8, 8, 8 epochs around an E-step"""
    c = MANAGERS[name]
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in c.get('env', {}).items():
        monkeypatch.setenv(k, v)
    if no_graph:
        monkeypatch.setenv('INVPREF_NO_GRAPH', '1')
    monkeypatch.setattr(_EpochEngine, '_SCHED_N', sched_n)
    U, I, E, D, n, bs, cls = (c[k] for k in ('U', 'I', 'E', 'D', 'n', 'bs', 'cls'))
    pure = cls is BasicImplicitTrainManager
    data = synth.interactions(41 + D, U, I, n, implicit=cls.implicit)
    tabs = synth.tables(42 + D, U, I, E, D, std=0.05)
    np.random.seed(5)
    td = torch.from_numpy(data).to(DEV)
    if pure:
        model = PureMatrixFactorization(U, I, D)
        model.load_state_dict({'user_emb.weight': torch.from_numpy(tabs[ops.PARAM_NAMES[0]]),
                               'item_emb.weight': torch.from_numpy(tabs[ops.PARAM_NAMES[1]])})
        mgr = cls(model, _Stub(), DEV, td, bs, 100, 10 ** 9, 0.005, 0.05, 0.01)
    else:
        model = (InvPrefImplicit if cls.implicit else InvPrefExplicit)(U, I, E, D, reg_only_embed=False, reg_env_embed=True)
        model.load_state_dict({k: torch.from_numpy(tabs[k]) for k in ops.PARAM_NAMES})
        mgr = cls(model=model, evaluator=_Stub(), device=DEV, training_data=td, batch_size=bs, epochs=100,
                  cluster_interval=100, evaluate_interval=10 ** 9, lr=0.005, invariant_coe=3.35, env_aware_coe=9.99,
                  env_coe=9.06, L2_coe=3.13, L1_coe=0.49, alpha=c.get('alpha', 1.9), use_class_re_weight=True,
                  use_recommend_re_weight=True, cluster_use_random_sort=False)
        assert mgr.update_alpha == (c.get('alpha', 1.9) is None)
    assert mgr.batch_num == 3 and n % bs != 0
    bases, trace, estep = [], [], None

    def note():
        bases.append(None if mgr._sched is None else mgr._sched['base'])

    if not pure:
        mgr.stat_envs()
        note()
    trace += mgr.train_epochs(1)
    note()
    for _ in range(2):
        trace += mgr.train_epochs(8)
        note()
    if not pure:
        estep = (mgr.cluster(), mgr.stat_envs())
        note()
    trace.append(mgr.train_a_epoch())
    note()
    trace += mgr.train_epochs(5)
    note()
    for _ in range(3):      # (three runs, not one: a table of 64 rows meets its second end, and third base, only in the last)
        trace += mgr.train_epochs(8)
        note()
    mgr.sync_parameters()
    assert bool(mgr._graphs) == (not no_graph)
    if 'alt' in c:
        assert (mgr._alt is not None) == c['alt']
    if 'INVPREF_UNFUSED' in c.get('env', {}):
        assert mgr._unfused
    assert mgr.epoch_cnt == len(trace) == 47 and mgr.state.step == 47 * 3
    st = mgr.state
    keys = list(trace[0])                     # (LOSS_KEYS; the PureMF managers report their own three)
    assert pure or keys == list(LOSS_KEYS)
    return dict(losses=np.array([[d[k] for k in keys] for d in trace]),
                params={k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()},
                moments=[st.exp_avg.cpu().numpy(), st.exp_avg_sq.cpu().numpy()], alpha=mgr.alpha, estep=estep,
                envs=None if pure else mgr.envs.cpu().numpy(), bases=[b for b in bases if b is not None])


_SHIPPED = {}


def _shipped(name: str, monkeypatch) -> dict:
    """the run with the shipped table (8192 rows: no refill at this length): once per configuration"""
    if name not in _SHIPPED:
        _SHIPPED[name] = _train(name, 8192, monkeypatch)
        assert len(set(_SHIPPED[name]['bases'])) == 1
    return _SHIPPED[name]


def _same_training(got: dict, want: dict):
    np.testing.assert_array_equal(got['losses'], want['losses'])
    assert np.isfinite(got['losses']).all()
    assert got['params'].keys() == want['params'].keys()
    for k in want['params']:
        np.testing.assert_array_equal(got['params'][k], want['params'][k], err_msg=k)
    for a, b in zip(got['moments'], want['moments']):
        np.testing.assert_array_equal(a, b)
    assert got['alpha'] == want['alpha']
    assert got['estep'] == want['estep']
    if want['envs'] is not None:
        np.testing.assert_array_equal(got['envs'], want['envs'])


# 24 rows: one replay of 8 epochs ends exactly on the last row; 32: a refill before almost every replay; 64: every few
@pytest.mark.parametrize('sched_n', [24, 32, 64])
@pytest.mark.parametrize('name', list(MANAGERS))
def test_training_does_not_depend_on_where_the_table_ends(name, sched_n, monkeypatch):
    want = _shipped(name, monkeypatch)
    got = _train(name, sched_n, monkeypatch)
    print(name, sched_n, 'bases', got['bases'])
    assert len(set(got['bases'])) >= 3          # (without this the test can pass without a single refill)
    _same_training(got, want)
    if MANAGERS[name].get('alpha', 1.9) is None:
        assert 0.99 < got['alpha'] < 1.0


def test_eager_epochs_equal_replayed_ones_two_launch_form(monkeypatch):
    """INVPREF_NO_GRAPH=1: the two-launch form issues the same launches eagerly, with explicit step numbers, that the graphs
    replay through the schedule -- bit for bit, whatever the table's length"""
    name = 'implicit_two_launch'
    eager = _train(name, 8192, monkeypatch, no_graph=True)
    assert eager['bases'] == []
    _same_training(eager, _shipped(name, monkeypatch))


def test_eager_epochs_equal_replayed_ones_alternating_form(monkeypatch):
    """The alternating form's eager epochs each end with a flush and start from the users' side again, so their sums run in
    another order than a replayed run's: held to what tests/test_manager_gpu.py holds graph replay against eager launches
    to (test_train_epochs_single_readback_equals_epoch_by_epoch, test_alpha_schedule_under_graph_replay)."""
    from test_manager_gpu import _assert_same_run
    name = 'implicit_alternating'
    eager = _train(name, 8192, monkeypatch, no_graph=True)
    assert eager['bases'] == []
    for sched_n in (8192, 24):
        got = _shipped(name, monkeypatch) if sched_n == 8192 else _train(name, sched_n, monkeypatch)
        print('alternating, eager vs replayed, table of', sched_n, 'rows: worst relative loss difference',
              float(np.abs(got['losses'] / eager['losses'] - 1).max()),
              'worst parameter difference', max(float(np.abs(got['params'][k] - eager['params'][k]).max()) for k in got['params']))
        np.testing.assert_allclose(got['losses'], eager['losses'], rtol=2e-6)
        for k in got['params']:
            _assert_same_run(np.abs(got['params'][k] - eager['params'][k]), 0.005, k)


def test_a_run_longer_than_the_table_is_refused(monkeypatch):
    """_sched_prepare(steps_ahead) refills when a run does not fit; a run longer than the table itself cannot be made to fit
    (its last steps would reuse stale scalars): InvPrefError, before anything is launched."""
    monkeypatch.setattr(_EpochEngine, '_SCHED_N', 16)
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    U, I, E, D = 300, 40, 4, 64
    data = synth.interactions(3, U, I, 2000, implicit=True)
    model = InvPrefImplicit(U, I, E, D, reg_only_embed=False, reg_env_embed=True)
    np.random.seed(5)
    mgr = ImplicitTrainManager(model=model, evaluator=_Stub(), device=DEV, training_data=torch.from_numpy(data).to(DEV),
                               batch_size=700, epochs=100, cluster_interval=100, evaluate_interval=10 ** 9, lr=0.005,
                               invariant_coe=1., env_aware_coe=1., env_coe=1., L2_coe=0.1, L1_coe=0.01, alpha=1.0,
                               cluster_use_random_sort=False)
    mgr.stat_envs()
    mgr.train_epochs(1)                       # the eager epoch
    assert mgr.graphs_enabled() and mgr._graph_epochs == 8
    before = [p.clone() for p in mgr.state.p_views]
    with pytest.raises(_capi.InvPrefError):
        mgr._sched_prepare(17)
    with pytest.raises(_capi.InvPrefError):
        mgr.train_epochs(8)                   # 24 steps in one replay, 16 rows
    assert mgr.epoch_cnt == 1 and mgr.state.step == 3
    for a, b in zip(before, mgr.state.p_views):
        assert torch.equal(a, b)
    mgr._sched_prepare(16)                    # a run of exactly the table's length fits
    assert mgr._sched['base'] == 4
    assert len(mgr.train_epochs(5)) == 5      # 15 steps
