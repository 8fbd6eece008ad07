"""PureMF baselines on the same fused HIP step: plain, propensity-weighted (IPS-MF, SNIPS-MF), ExpoMF, WMF,
CVIB-MF and fairness-MF; and MACR-MF, LinearTrans-MF, CausE, BPR-MF and doubly robust MF, whose steps are gradient passes of
their own (csrc/invpref_macr.hip, csrc/invpref_lintrans.hip, csrc/invpref_cause.hip, csrc/invpref_bpr.hip, csrc/invpref_dr.hip),
sampled-softmax MF (csrc/invpref_ssm.hip), LightGCN, whose propagation is csrc/invpref_lgcn.hip and whose step is BPR's, and
DICE, whose popularity-margin draw and four-table pass are csrc/invpref_dice.hip; and EASE, the item-item ridge model in closed
form (csrc/invpref_ease.hip), which has no embedding tables at all.

Drop-in for the reference's ``PureMatrixFactorization`` / ``PureExplicitMatrixFactorization``
(baseline_models.py:12-69, :652-704) and ``Basic{Implicit,Explicit}TrainManager`` /
``BasicUniform*TrainManager`` (train.py:345-481, :1022-1157): same constructor signatures, attribute and
parameter names (``user_emb.weight``, ``item_emb.weight``), loss-dict keys and return shapes.

PureMF is the degenerate case of the InvPref step: with the env-aware tables, ``embed_env`` and the
classifier absent (``INVPREF_PURE_MF``: never loaded, never stored), one environment and coefficients
``(1, 0, 0, 2*L2_coe, 2*L1_coe, alpha=0)`` the InvPref loss IS ``score_loss + L2_coe*L2_reg + L1_coe*L1_reg``
of train.py:389-397 (the InvPref regularisers are normalised by 2*B*D, PureMF's by B*D; see
oracle/oracle.py ``pure_mf_*`` for the CPU statement of the same mapping, pinned by goldens g7).  The
managers are built on the epoch engine of ``engine.py`` (row plans, fused Adam, HIP-graph replay, deferred read-backs).

IPS-MF / SNIPS-MF (baseline_train.py:317-581, :800-976) are the same step with a fixed per-interaction weight on the score
loss (``INVPREF_REWEIGHT_REC``): the inverse propensities are formed once on the device (csrc/invpref_propensity.hip), and
SNIPS's per-minibatch normaliser sum(w) is folded into the weights of the static minibatches (w' = w * B_b / S_b).
"""
from __future__ import annotations

import numpy as np
import torch
from torch import nn

from . import _capi, ops
from . import plan as planlib
from .engine import _EpochEngine, _OuterLoop

PURE_LOSS_KEYS = ['score_loss', 'L2_reg', 'L1_reg', 'loss']  # train.py:399-404


class _PureMFBase(nn.Module):
    implicit = True

    def __init__(self, user_num: int, item_num: int, factor_num: int):
        super().__init__()
        self.user_num, self.item_num, self.factor_num = user_num, item_num, factor_num
        self.user_emb = nn.Embedding(user_num, factor_num)
        self.item_emb = nn.Embedding(item_num, factor_num)
        nn.init.normal_(self.user_emb.weight, std=0.01)  # baseline_models.py:23-25
        nn.init.normal_(self.item_emb.weight, std=0.01)
        self._absent = None

    def tables(self):
        return [self.user_emb.weight, self.item_emb.weight]

    # ---- unfused, autograd-capable surface (what the reference's untouched Basic*TrainManager calls).
    # It goes through the InvPref forward / backward kernels with zero stand-ins for the absent tables
    # (allocated on first use; the managers below never need them).
    def _seven(self):
        w = self.user_emb.weight
        if self._absent is None or self._absent[0].device != w.device:
            z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=w.device)  # noqa: E731
            D = self.factor_num
            self._absent = [z(self.user_num, D), z(self.item_num, D), z(1, D), z(1, D), z(1)]
        return [self.user_emb.weight, self.item_emb.weight] + self._absent

    def _scores(self, users_id, items_id):
        from .autograd import InvPrefForward
        inv, _, _ = InvPrefForward.apply(users_id, items_id, torch.zeros_like(users_id), 0., self.implicit, *self._seven())
        return inv

    def forward(self, users_id, items_id, ground_truth=None):  # baseline_models.py:27-37 / :665-674
        final_ratings = self._scores(users_id, items_id)
        if ground_truth is not None:
            return self.loss_func(final_ratings, ground_truth)
        return final_ratings

    def _reg(self, users_id, items_id, norm: int):
        # InvPref's regulariser over (Pu, Pa=0) and (Qi, Qa=0) is normalised by 2*B*D: PureMF's is twice that
        from .autograd import InvPrefReg
        return 2. * InvPrefReg.apply(users_id, items_id, torch.zeros_like(users_id), norm, True, False, *self._seven())

    def get_L1_reg(self, users_id, items_id):  # baseline_models.py:59-60
        return self._reg(users_id, items_id, 1)

    def get_L2_reg(self, users_id, items_id):  # baseline_models.py:62-63
        return self._reg(users_id, items_id, 2)


class PureMatrixFactorization(_PureMFBase):
    """baseline_models.py:12-69"""
    implicit = True

    def __init__(self, user_num: int, item_num: int, factor_num: int):
        super().__init__(user_num, item_num, factor_num)
        self.output_func = nn.Sigmoid()
        self.loss_func = nn.BCELoss()

    def predict(self, users_id):  # baseline_models.py:65-69: sigmoid(Pu[users] @ Qi^T)
        from .autograd import predict_all_items
        return predict_all_items(self.user_emb.weight.detach(), self.item_emb.weight.detach(), users_id, sigmoid=True)

    def recommend(self, users_id, k: int, exclude=None, highlight=None):
        """Each user's top-k items by the scores of predict() (InvPrefImplicit.recommend)."""
        t = self.tables()
        return ops.recommend(t[0], t[1], users_id, k, exclude, highlight)


class PureExplicitMatrixFactorization(_PureMFBase):
    """baseline_models.py:652-704"""
    implicit = False

    def __init__(self, user_num: int, item_num: int, factor_num: int):
        super().__init__(user_num, item_num, factor_num)
        self.loss_func = nn.MSELoss()

    def predict(self, users_id, items_id):  # baseline_models.py:703-704
        with torch.no_grad():
            return self._scores(users_id, items_id).reshape(-1)


class _BasicTrainManager(_EpochEngine):
    """Basic{Implicit,Explicit}TrainManager (train.py:345-461, :1022-1138) on the fused PureMF step: the epoch engine as it
    is (engine.py: every hook's default is PureMF's answer) + the coefficients, the four loss keys and train_a_batch."""

    def __init__(self, model, evaluator, device: torch.device, training_data: torch.Tensor, batch_size: int,
                 epochs: int, evaluate_interval: int, lr: float, L2_coe: float, L1_coe: float,
                 test_begin_epoch: int = 0, *, rank=None, world_size=None, process_group=None):
        """rank / world_size / process_group (keyword-only, beyond the reference's signature): one process per GPU,
        sharded like the InvPref managers (parallel.py; INVPREF_SHARD=users|rows): every rank keeps its share of
        every minibatch, one all-reduce per optimiser step, every mean() over the GLOBAL minibatch."""
        self._init_engine(model, evaluator, device, training_data, batch_size, epochs, evaluate_interval, lr, L2_coe, L1_coe,
                          test_begin_epoch, rank, world_size, process_group,
                          flags=ops.flags_of(self.implicit, False, False, True, False, dense_reg=False) | _capi.PURE_MF,
                          users_first=None,     # [user table | item table]: the shared part is last as listed
                          env_switches=False)

    _LOSS_KEYS = PURE_LOSS_KEYS     # (train.py:399-404)

    def _coefs(self, alpha):
        return (1., 0., 0., 2. * self.L2_coe, 2. * self.L1_coe, 0.)

    @staticmethod
    def loss_dicts(dev_losses: torch.Tensor) -> list:
        """InvPref's six outputs -> the four PureMF terms (the regulariser reports are twice InvPref's)."""
        return [dict(zip(PURE_LOSS_KEYS, (v[0], 2. * v[3], 2. * v[4], v[5]))) for v in dev_losses.tolist()]

    def train_a_batch(self, batch_users_tensor, batch_items_tensor, batch_scores_tensor, *args) -> dict:
        """train.py:379-405 on caller-supplied tensors: the row plan of this one minibatch is built on the
        host first (the epoch loop uses the plans prepared once for the static minibatches instead).
        Single-process form; sharded runs go through train_epochs() / train()."""
        return self._batch_step(batch_users_tensor, batch_items_tensor, batch_scores_tensor, None)

    def _batch_step(self, batch_users, batch_items, batch_scores_tensor, weights, term=None) -> dict:
        """one step on caller-supplied ids (tensors or host arrays) and labels; weights (fp32, device, one per interaction) are
        read under INVPREF_REWEIGHT_REC, None runs the unweighted step.  term None: the fused step.  term, a callable that adds
        a further loss term's gradient into state.g_views and its value into state.losses6: the unfused sequence, gradient
        pass -> term() -> Adam over this rank's ranges."""
        if self.world_size > 1:
            raise NotImplementedError('train_a_batch on caller-supplied tensors is single-process; use train_epochs()')
        flags = self._flags if weights is not None else self._flags & ~_capi.REWEIGHT_REC
        u, v = (x if isinstance(x, np.ndarray) else x.detach().cpu().numpy() for x in (batch_users, batch_items))
        y = batch_scores_tensor.detach().float().contiguous()
        dp = self._batch_plan(u, v, y.cpu().numpy())
        st = self.state
        st.losses6.zero_()
        st.step += 1
        self._sched_synced = False
        if term is None and self._lazy:
            # lazy Adam (set_lazy_adam): the gradient pass over the touched rows only, then Adam on them
            rows = self._lazy_batch_rows(u, v)
            self._gradient_pass(None, planlib.without_streamed_rows(dp), None, None, None, y.to(self.device), weights, len(u),
                                self._coefs(0.), flags, st.losses6)
            self._lazy_adam(rows)
        elif term is None:
            ops.mstep_rows_adam(st.p_views, st.p_views_alt, st.m_views, st.v_views, dp, None, y.to(self.device), weights,
                                len(u), self._coefs(0.), flags, st.losses6, st.step, self.lr, self.workspace,
                                pure=True)
            st.swap()
        else:
            self._gradient_pass(None, dp, None, None, None, y.to(self.device), weights, len(u), self._coefs(0.), flags,
                                st.losses6)
            term()
            self._grad_stale = True     # (the planned pass overwrote every row: nothing to zero, see _step())
            for o, ln in self._adam_ranges:
                ops.adam_(st.param[o:o + ln], st.grad[o:o + ln], st.exp_avg[o:o + ln], st.exp_avg_sq[o:o + ln], st.step,
                          self.lr, zero_grad=False)
        return self.loss_dicts(st.losses6[None])[0]


class BasicImplicitTrainManager(_BasicTrainManager):
    """reference train.py:345-461 (BCELoss)"""
    implicit = True


class BasicExplicitTrainManager(_BasicTrainManager):
    """reference train.py:1022-1138 (MSELoss)"""
    implicit = False


class _UniformMixin:
    def _keep_uniform(self, uniform_data):  # train.py:478-481 / :1154-1157: stored, not used by the loop
        self.uniform_user = uniform_data[:, 0].to(self.device).long()
        self.uniform_item = uniform_data[:, 1].to(self.device).long()
        self.uniform_score = uniform_data[:, 2].to(self.device).float()


class BasicUniformImplicitTrainManager(BasicImplicitTrainManager, _UniformMixin):
    """reference train.py:464-481"""

    def __init__(self, model, evaluator, device, training_data, uniform_data, batch_size, epochs, evaluate_interval,
                 lr, L2_coe, L1_coe, test_begin_epoch: int = 0):
        super().__init__(model, evaluator, device, training_data, batch_size, epochs, evaluate_interval, lr, L2_coe,
                         L1_coe, test_begin_epoch)
        self._keep_uniform(uniform_data)


class BasicUniformExplicitTrainManager(BasicExplicitTrainManager, _UniformMixin):
    """reference train.py:1140-1157"""

    def __init__(self, model, evaluator, device, training_data, uniform_data, batch_size, epochs, evaluate_interval,
                 lr, L2_coe, L1_coe, test_begin_epoch: int = 0):
        super().__init__(model, evaluator, device, training_data, batch_size, epochs, evaluate_interval, lr, L2_coe,
                         L1_coe, test_begin_epoch)
        self._keep_uniform(uniform_data)


# ------------------------------------------------------------------------------------------------ IPS-MF / SNIPS-MF
def _f32_device(a, device) -> torch.Tensor:
    """torch.Tensor(np_array).to(device) of baseline_train.py:382: one rounding to fp32"""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1)).astype(np.float32)).to(device)


def _count_propensity_np(kind, user_inter_cnt_np, item_inter_cnt_np, interactions, smooth_weight_coe):
    dev = torch.device('cuda', torch.cuda.current_device())
    inter = np.asarray(interactions)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a).reshape(-1), dtype=np.int64)).to(dev)  # noqa: E731
    cnt = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64).reshape(-1)).to(dev)  # noqa: E731
    w = ops.count_propensity(cnt(user_inter_cnt_np) if kind != _capi.PROPENSITY_ITEM else None,
                             cnt(item_inter_cnt_np) if kind != _capi.PROPENSITY_USER else None,
                             up(inter[:, 0]) if kind != _capi.PROPENSITY_ITEM else None,
                             up(inter[:, 1]) if kind != _capi.PROPENSITY_USER else None, kind, smooth_weight_coe)
    return w.cpu().numpy()


def basic_item_propensity_func(user_inter_cnt_np, item_inter_cnt_np, interactions, smooth_weight_coe: float) -> np.ndarray:
    """baseline_train.py:493-505 on the device: (1 / (item_cnt / max item_cnt))[item] ** smooth_weight_coe, as the fp32
    values the managers upload (torch.Tensor(np_array), baseline_train.py:382)"""
    return _count_propensity_np(_capi.PROPENSITY_ITEM, user_inter_cnt_np, item_inter_cnt_np, interactions, smooth_weight_coe)


def basic_user_propensity_func(user_inter_cnt_np, item_inter_cnt_np, interactions, smooth_weight_coe: float) -> np.ndarray:
    """baseline_train.py:508-520 on the device (fp32 result)"""
    return _count_propensity_np(_capi.PROPENSITY_USER, user_inter_cnt_np, item_inter_cnt_np, interactions, smooth_weight_coe)


def basic_pair_propensity_func(user_inter_cnt_np, item_inter_cnt_np, interactions, smooth_weight_coe: float) -> np.ndarray:
    """baseline_train.py:523-546 on the device: ((inv_u + inv_i) / 2) ** smooth_weight_coe (fp32 result)"""
    return _count_propensity_np(_capi.PROPENSITY_PAIR, user_inter_cnt_np, item_inter_cnt_np, interactions, smooth_weight_coe)


def naive_bayes_propensity(train_data, uniform_data, user_num: int, item_num: int, smooth_weight_coe: float) -> np.ndarray:
    """baseline_train.py:549-581 on the device: the weight of every training interaction's label (fp32 result; a label absent
    from the uniform sample weighs 0)"""
    dev = torch.device('cuda', torch.cuda.current_device())
    col = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a)[:, 2], dtype=np.float32)).to(dev)  # noqa: E731
    w, _ = ops.naive_bayes_propensity(col(train_data), col(uniform_data), user_num, item_num, smooth_weight_coe)
    return w.cpu().numpy()


_COUNT_KINDS = {basic_item_propensity_func: _capi.PROPENSITY_ITEM, basic_user_propensity_func: _capi.PROPENSITY_USER,
                basic_pair_propensity_func: _capi.PROPENSITY_PAIR}


class _PropensityMixin(_UniformMixin):
    """IPSBasicTrainManager / SNIPSMFTrainManager and their explicit twins (baseline_train.py:317-491, :800-976) on the
    fused PureMF step with INVPREF_REWEIGHT_REC.  The weights are counted over the GLOBAL training data before the rows
    are sharded and then follow this rank's rows; SNIPS's normaliser is folded into them per GLOBAL minibatch."""
    _snips = False

    def __init__(self, model, propensity_func, evaluator, device, training_data: torch.Tensor, batch_size: int,
                 epochs: int, evaluate_interval: int, lr: float, L2_coe: float, L1_coe: float, test_begin_epoch: int = 0,
                 smooth_weight_coe: float = 1.0, uniform_data: torch.Tensor = None, *, rank=None, world_size=None,
                 process_group=None):
        super().__init__(model, evaluator, device, training_data, batch_size, epochs, evaluate_interval, lr, L2_coe,
                         L1_coe, test_begin_epoch, rank=rank, world_size=world_size, process_group=process_group)
        self.loss_func = nn.BCELoss(reduction='none') if self.implicit else nn.MSELoss(reduction='none')
        self.smooth_weight_coe = smooth_weight_coe
        self.propensity_func = propensity_func
        dev, U, I = self.device, model.user_num, model.item_num
        users = training_data[:, 0].to(dev).long().contiguous()     # every row, in order (not this rank's share)
        items = training_data[:, 1].to(dev).long().contiguous()
        self._cnt_dev = ops.interaction_counts(users, items, U, I)  # baseline_train.py:335-348
        self._cnt_np = [None, None]
        if uniform_data is not None:
            self._keep_uniform(uniform_data)
            if propensity_func is naive_bayes_propensity:
                w, _ = ops.naive_bayes_propensity(training_data[:, 2].to(dev), self.uniform_score, U, I, smooth_weight_coe)
            else:
                w = _f32_device(propensity_func(training_data.cpu().detach().numpy(), uniform_data.cpu().detach().numpy(),
                                                U, I, smooth_weight_coe), dev)
        elif propensity_func in _COUNT_KINDS:
            w = ops.count_propensity(*self._cnt_dev, users, items, _COUNT_KINDS[propensity_func], smooth_weight_coe)
        else:
            inter = np.stack([users.cpu().numpy(), items.cpu().numpy()], axis=1)
            w = _f32_device(propensity_func(self.user_inter_cnt_np, self.item_inter_cnt_np, inter, smooth_weight_coe), dev)
        if w.numel() != self.n_total:
            raise ValueError(f'propensity_func returned {w.numel()} weights for {self.n_total} interactions')
        self.inverse_propensity_tensor = w
        # what the epochs' launches read: SNIPS-scaled per global minibatch, then this rank's rows
        w = ops.snips_scale(w, batch_size) if self._snips else w
        self._w_local = w.index_select(0, self.shard.local_rows().to(dev)) if self.world_size > 1 else w
        self._flags |= _capi.REWEIGHT_REC

    def _cnt(self, i):
        if self._cnt_np[i] is None:
            self._cnt_np[i] = self._cnt_dev[i].cpu().numpy()
        return self._cnt_np[i]

    @property
    def user_inter_cnt_np(self) -> np.ndarray:
        """float64 [user_num]: clip(interactions per user, 1, max) (baseline_train.py:335-347), read back on first use"""
        return self._cnt(0)

    @user_inter_cnt_np.setter
    def user_inter_cnt_np(self, value):
        self._cnt_np[0] = value

    @property
    def item_inter_cnt_np(self) -> np.ndarray:
        return self._cnt(1)

    @item_inter_cnt_np.setter
    def item_inter_cnt_np(self, value):
        self._cnt_np[1] = value

    def _pure_weights(self, lo: int, hi: int):
        return self._w_local[lo:hi]

    def train_a_batch(self, batch_users_tensor, batch_items_tensor, batch_scores_tensor, weight_tensor=None) -> dict:
        """baseline_train.py:385-416 / :457-491: mean(loss * w) (IPS) or sum(loss * w) / sum(w) (SNIPS) on caller tensors;
        without weights both are the plain PureMF step."""
        w = None
        if weight_tensor is not None:
            w = weight_tensor.detach().to(self.device).float().reshape(-1).contiguous()
            if self._snips:
                w = ops.snips_scale(w, max(w.numel(), 1))
        return self._batch_step(batch_users_tensor, batch_items_tensor, batch_scores_tensor, w)


class IPSBasicTrainManager(_PropensityMixin, BasicImplicitTrainManager):
    """reference baseline_train.py:317-436 (BCELoss, mean(loss * inverse propensity))"""


class SNIPSMFTrainManager(IPSBasicTrainManager):
    """reference baseline_train.py:439-490 (sum(loss * w) / sum(w) per minibatch)"""
    _snips = True


class IPSBasicExplicitTrainManager(_PropensityMixin, BasicExplicitTrainManager):
    """reference baseline_train.py:800-921 (MSELoss)"""


class SNIPSExplicitMFTrainManager(IPSBasicExplicitTrainManager):
    """reference baseline_train.py:924-976"""
    _snips = True


# ------------------------------------------------------------------------------------------------ ExpoMF
class ExposureMatrixFactorization(PureMatrixFactorization):
    """baseline_models.py:237-256: PureMF with per-interaction BCE losses and the exposure posterior.  Same parameters and
    initialisation; ImplicitTestManager ranks it through the fused route like any PureMatrixFactorization."""

    def __init__(self, user_num: int, item_num: int, factor_num: int):
        super().__init__(user_num, item_num, factor_num)
        self.loss_func = nn.BCELoss(reduction='none')

    def forward(self, users_id, items_id, ground_truth):  # baseline_models.py:244-250: one loss per interaction
        return self.loss_func(self._scores(users_id, items_id), ground_truth)

    def calculate_exposure_probability(self, user_id, lam_y: float, mu, eps: float) -> torch.Tensor:
        """baseline_models.py:252-256: the detached fp32 posterior [n, I] of the given users on the device (the store mode of
        csrc/invpref_exposure.hip's pass)"""
        P, Q = self.user_emb.weight.detach(), self.item_emb.weight.detach()
        mu = torch.as_tensor(mu).to(device=P.device, dtype=torch.float32).reshape(-1).contiguous()
        return ops.exposure_probability(P, Q, torch.as_tensor(user_id).to(P.device), mu, lam_y, eps)


def _zero_pow(e: float) -> float:
    """an entry of the reference's float64 np.zeros matrix ** e (what every weight is before the first recompute)"""
    with np.errstate(divide='ignore'):
        return float(np.float64(0.0) ** e)


class ExpoMFTrainManager(BasicImplicitTrainManager):
    """reference baseline_train.py:16-154 on the fused PureMF step with INVPREF_REWEIGHT_REC: the loss is
    mean(BCE * w) + the PureMF regularisers, w = prob ** expo_weight_exp at the minibatch's pairs (1.0 at pairs with a
    positive training row).

    The reference keeps the posterior as a dense [U, I] host array, rebuilt every upd_expo_interval epochs, gathered and
    copied to the device at every step.  Here nothing U x I exists during training:
      - every recompute copies the two tables and mu into a device snapshot and refreshes ONE fp32[N] weight buffer in place
        (the epochs' launches read slices of it, so the captured epoch graphs stay valid);
      - the prior update after every epoch is one exposure pass whose epilogue reduces to per-item float64 column sums,
        updating the device buffer mu in place.
    ``exposure_probability`` materialises the reference's matrix from the snapshot on request only."""
    _lazy_adam_unsupported = 'lazy Adam is not built for ExpoMF, whose posterior and prior passes surround runs of the fused step'

    def __init__(self, model, evaluator, device, training_data: torch.Tensor, batch_size: int, epochs: int,
                 evaluate_interval: int, lr: float, L2_coe: float, L1_coe: float, test_begin_epoch: int = 0,
                 lam_y: float = 1.0, init_mu: float = 1e-2, a: float = 1.0, b: float = 1.0, expo_weight_exp: float = 1.0,
                 eps: float = 1e-8, upd_expo_interval: int = 10, *, rank=None, world_size=None, process_group=None):
        if int(upd_expo_interval) < 1:
            raise ValueError(f'upd_expo_interval must be at least 1, got {upd_expo_interval}')
        super().__init__(model, evaluator, device, training_data, batch_size, epochs, evaluate_interval, lr, L2_coe, L1_coe,
                         test_begin_epoch, rank=rank, world_size=world_size, process_group=process_group)
        if self.world_size > 1:
            raise NotImplementedError('ExpoMF runs on one GPU (a sharded exposure pass is not implemented)')
        self.model = model
        self.lam_y, self.a, self.b = float(lam_y), float(a), float(b)
        self.expo_weight_exp, self.eps = float(expo_weight_exp), float(eps)
        self.upd_expo_interval = int(upd_expo_interval)
        dev, U, I = self.device, model.user_num, model.item_num
        self._mu = torch.full((I,), float(init_mu), dtype=torch.float32, device=dev)   # torch.Tensor(init_mu * ones): fp32
        self.user_id_tensor = torch.arange(U, dtype=torch.int64, device=dev)
        # a row is positive when ANY training row of its (u, i) has a nonzero label (baseline_train.py:57-61)
        keys = self.users_tensor * I + self.items_tensor
        self._pos_keys = torch.unique(keys[self.scores_tensor != 0])           # sorted
        self._positive = torch.isin(keys, self._pos_keys)
        # the reference's np.zeros matrix before the first recompute: every weight is 0.0 ** e
        self._w = torch.full((self.n_total,), _zero_pow(self.expo_weight_exp), dtype=torch.float32, device=dev)
        P, Q = self.state.p_views[0], self.state.p_views[1]
        self._snap = (torch.empty_like(P), torch.empty_like(Q), torch.empty_like(self._mu))
        self._snapped = False
        self._expo_ws = ops.Workspace(dev)
        self._expo_ws.get(max(ops.exposure_workspace_bytes(U, I), 1))           # sized once: graph-capturable passes
        self._flags |= _capi.REWEIGHT_REC

    @property
    def mu(self) -> torch.Tensor:
        """the item priors: a device fp32 [item_num] buffer, updated in place"""
        return self._mu

    @mu.setter
    def mu(self, value):
        self._mu.copy_(torch.as_tensor(value).reshape(-1))

    def _pure_weights(self, lo: int, hi: int):
        return self._w[lo:hi]

    def calculate_exposure_probability(self):
        """baseline_train.py:43-61: snapshot the tables and mu, then refresh the weights of every training row (positives 1.0)
        in place.  Enqueued on the current stream; nothing is read back."""
        self.model.eval()
        P, Q = self.state.p_views[0], self.state.p_views[1]
        for dst, src in zip(self._snap, (P, Q, self._mu)):
            dst.copy_(src)
        self._snapped = True
        sP, sQ, smu = self._snap
        ops.exposure_weights(sP, sQ, self.users_tensor, self.items_tensor, self._positive, smu, self.lam_y, self.eps,
                             self.expo_weight_exp, out=self._w)

    def upd_mu(self):
        """baseline_train.py:63-79: mu <- (a + sum_u prob(u, i) - 1) / (a + b + U - 2) over every user, from the current tables
        and mu (no positive override), in place.  One exposure pass + a fold; nothing [U, I] is stored."""
        self.model.eval()
        ops.exposure_prior_(self.state.p_views[0], self.state.p_views[1], None, self._mu, self.lam_y, self.eps, self.a, self.b,
                            self._expo_ws)

    @property
    def exposure_probability(self) -> np.ndarray:
        """The reference's [U, I] matrix (baseline_train.py:40, :55-61), materialised from the last recompute's snapshot in
        chunks of users, positives set to 1.0: float32, or float64 zeros before the first recompute.  Costs U * I * 4 bytes of
        host memory and as much device traffic -- for inspection; training never builds it."""
        U, I = self.model.user_num, self.model.item_num
        if not self._snapped:
            return np.zeros([U, I])
        sP, sQ, smu = self._snap
        out = np.empty((U, I), dtype=np.float32)
        step = max(1, min(U, (64 << 20) // (4 * I)))
        for lo in range(0, U, step):
            hi = min(U, lo + step)
            out[lo:hi] = ops.exposure_probability(sP, sQ, self.user_id_tensor[lo:hi], smu, self.lam_y, self.eps).cpu().numpy()
        k = self._pos_keys.cpu().numpy()
        out[k // I, k % I] = 1.0
        return out

    def train_a_batch(self, batch_users_tensor, batch_items_tensor, batch_scores_tensor) -> dict:
        """baseline_train.py:81-116 on caller tensors: the weights of ANY pair from the last recompute's snapshot (1.0 at pairs
        with a positive training row), or 0.0 ** e before the first recompute."""
        u = batch_users_tensor.detach().to(self.device).long().reshape(-1).contiguous()
        v = batch_items_tensor.detach().to(self.device).long().reshape(-1).contiguous()
        if not self._snapped:
            w = torch.full((u.numel(),), _zero_pow(self.expo_weight_exp), dtype=torch.float32, device=self.device)
        else:
            pos = torch.isin(u * self.model.item_num + v, self._pos_keys)
            sP, sQ, smu = self._snap
            w = ops.exposure_weights(sP, sQ, u, v, pos, smu, self.lam_y, self.eps, self.expo_weight_exp)
        return self._batch_step(u, v, batch_scores_tensor, w)

    # baseline_train.py:118-154 on the engine's outer loop: one-epoch runs (graph replays; the alternating form flushes at the
    # end of each, so the tables are consistent between runs), the weight refresh enqueued before the due epochs, the prior
    # update after every run.  silent / auto: no per-epoch host sync.
    def _epochs_to_next_event(self) -> int:
        return 1

    def _before_run(self) -> None:
        if self.epoch_cnt % self.upd_expo_interval == 0:
            self.calculate_exposure_probability()

    def _after_run(self) -> None:
        self.upd_mu()


# ------------------------------------------------------------------------------------------------ drawn terms
class _SingleProcessMixin:
    _SINGLE = None                  # why the manager runs in a single process

    def _require_single_process(self, world_size) -> None:
        """called with the constructor's argument before the engine is built, and with the resolved size after"""
        if world_size is not None and int(world_size) > 1:
            raise NotImplementedError(self._SINGLE)


class _StagedRunMixin(_SingleProcessMixin):
    """A step that reads ids DRAWN anew for every step, in front of a _BasicTrainManager: always the engine's unfused sequence,
    gradient pass -> _after_gradient_pass -> dense / ranged Adam.  Single process.  Before a run of epochs is enqueued the
    draws of all its steps are staged in ONE device int32 buffer, row = the step's position in the run.  The launches read
    their row when they run, so a captured run of epochs is replayed with new draws without re-capture.

    A layer above supplies _stage_draws(n), the draws of the next n epochs' steps into the first rows, stream-ordered (a copy
    of host draws: _DrawnTermMixin; a draw launch: _DeviceDrawnMixin), and _draws_consumed(steps), told how many were issued."""

    def _init_staging(self, width: int) -> None:
        self._require_single_process(self.world_size)
        self._unfused = True        # (never the fused / alternating step)
        self._row_width = width
        self._staged = None         # device int32 [steps of the longest run, width]

    def _limit_run(self) -> None:
        """may lower self._graph_epochs before the staging buffer is sized for it"""

    def _staging_resized(self, rows: int) -> None:
        """the staging buffer was (re)allocated with `rows` rows: size what goes with it"""

    def _raw_setup(self):
        super()._raw_setup()
        self._limit_run()
        rows = self._graph_epochs * self.batch_num
        if self._staged is None or self._staged.shape[0] != rows:
            self._staged = torch.zeros(rows, self._row_width, dtype=torch.int32, device=self.device)
            self._staging_resized(rows)

    def _enqueue_epochs(self, want: int) -> torch.Tensor:
        n = min(want, self._graph_epochs) if (self.graphs_enabled() and self._graph_warm) else 1
        self._stage_draws(n)
        before = self.epoch_cnt
        out = super()._enqueue_epochs(want)
        self._draws_consumed((self.epoch_cnt - before) * self.batch_num)   # (a failed capture runs one eager epoch of the n)
        return out

    def prepare_graphs(self, run_lengths) -> None:
        if self._staged is None:
            raise RuntimeError('prepare_graphs(): run one epoch first (train_epochs(1))')
        super().prepare_graphs(run_lengths)


class _DrawnTermMixin(_StagedRunMixin):
    """A PureMF step with one further loss term over ids drawn per step on the HOST (the WMF, fairness and CVIB managers
    below): the staged step of _StagedRunMixin with one call between the gradient pass and Adam, planned PureMF gradient pass
    -> the term (adds into the same gradient buffer and into the step's `loss`) -> Adam.

    A draw is a pair of id arrays (one array under _ONE_ARRAY).  The minibatches are static, so what every step draws from is
    listed once (_draw_specs); a run's draws are made on the host in the reference's order and go to the device in one copy.
    The draw source replaces numpy's global generator: a callable taking _draw_default's arguments, called once per step in
    order, or an iterable of pairs consumed in that order (recorded draws).

    A manager supplies: _SINGLE and _WHAT (the error texts), _draw_default, _draw_specs, _row_layout, _term(), and, where the
    staged rows need a pass of their own on the device, _after_staging()."""
    _WHAT = None                    # what a draw is called in the size check's error
    _draw_default = None            # staticmethod: one step's draw from numpy's global generator
    _ONE_ARRAY = False              # a draw is ONE id array (the pair's second stays empty: lengths (n, 0))
    _lazy_adam_unsupported = 'the drawn term adds gradient to rows outside the minibatch, which lazy Adam would not update'

    def _init_draws(self, source, specs, second_at: int, width: int) -> None:
        """source: the constructor's keyword; specs: per static minibatch (the arguments of its draw, the lengths (first,
        second) a draw of it must have); second_at / width: a staging row holds the first array from 0 and the second from
        second_at, zero-padded to width"""
        self._init_staging(width)
        self._draw_source = source
        self._draw_iter = iter(source) if source is not None and not callable(source) else None
        self._draw_specs, self._row_layout = specs, (second_at, width)
        self._queue = []            # drawn, not yet consumed: whole epochs of pairs in step order

    def _draw(self, args, want):
        if self._draw_source is None:
            d = self._draw_default(*args)
        elif self._draw_iter is not None:
            d = next(self._draw_iter)
        else:
            d = self._draw_source(*args)
        a, b = (d, np.zeros(0, np.int32)) if self._ONE_ARRAY else d
        a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
        if (len(a), len(b)) != want:
            if self._ONE_ARRAY:
                raise ValueError(f'a {self._WHAT} of {len(a)} ids where the step takes {want[0]}')
            raise ValueError(f'a {self._WHAT} of {len(a)} and {len(b)} ids where the step takes {want[0]} and {want[1]}')
        return a.astype(np.int32), b.astype(np.int32)

    def _after_staging(self, steps: int) -> None:
        """enqueued behind the copy of a run's first `steps` rows"""

    def _stage_draws(self, n: int):
        """the draws of the next n epochs: made (those not yet made), laid out one row per step, one copy"""
        steps = n * self.batch_num
        while len(self._queue) < steps:
            self._queue.extend(self._draw(args, want) for args, want in self._draw_specs)
        at, width = self._row_layout
        host = np.zeros((steps, width), np.int32)
        for s in range(steps):
            a, b = self._queue[s]
            host[s, :len(a)] = a
            host[s, at:at + len(b)] = b
        src = torch.from_numpy(host)
        if self._staged.is_cuda:
            src = src.pin_memory()
        self._staged[:steps].copy_(src, non_blocking=True)
        self._after_staging(steps)

    def _draws_consumed(self, steps: int) -> None:
        del self._queue[:steps]

    def _after_gradient_pass(self, k: int, losses6: torch.Tensor) -> None:
        self._term(k, self._loss_slot * self.batch_num + k, losses6[5:6])

    def _term(self, k: int, s: int, loss: torch.Tensor) -> None:
        """the term of static minibatch k from staging row s: gradient into state.g_views, value added into loss"""
        raise NotImplementedError


class _RunIndexMixin(_StagedRunMixin):
    """A run's drawn PAIRS and their inverted index on the device, for the passes built on csrc/chunk_walk.hpp (CVIB, BPR,
    doubly robust MF): a step takes as many drawn pairs as its minibatch has rows.  A staging row is the pair's two id arrays
    of `_cap` entries each, the longest minibatch's rows: `_draws` views the buffer as [rows, 2, _cap].  Behind the staging of
    a run's draws _index_run() indexes them in ONE batched pass (ops.cvib_index: destination row -> positions of the
    minibatch's pairs and the drawn pairs together) into `_index`, [rows, 2, 2 _cap, 2]; `_step_lo` / `_step_n` say which rows
    of the training data a step's minibatch is.  The captured launches read their row of both buffers when they run.

    A manager supplies _workspace_bytes(batch), the ops.*_workspace_bytes of its pass over a minibatch of `batch` rows."""
    # bytes of the run's index: longer runs are replayed as several shorter graphs.  Building it takes twice as much for a
    # moment (the keys and the alternate buffer of their in-place sort: ops.cvib_index), freed before the run starts
    _INDEX_BUDGET = 512 << 20

    def _init_run_index(self) -> None:
        n, bs = self.n_total, self.batch_size
        self._batch_lens = [min(bs, n - lo) for lo in range(0, n, bs)]
        self._cap = max(self._batch_lens)
        self._draws = self._index = None
        self._ws = ops.Workspace(self.device)
        self._ws.get(max(self._workspace_bytes(self._cap), 16))   # sized once: capturable launches

    def _limit_run(self) -> None:
        per_epoch = self.batch_num * self._cap * 32          # int32 (row, position) x two sides x 2 B entries per step
        self._graph_epochs = max(1, min(self._graph_epochs, self._INDEX_BUDGET // per_epoch))

    def _staging_resized(self, rows: int) -> None:
        dev = self.device
        self._draws = self._staged.view(rows, 2, self._cap)
        self._index = torch.zeros(rows, 2, 2 * self._cap, 2, dtype=torch.int32, device=dev)
        lo = np.arange(self.batch_num, dtype=np.int64) * self.batch_size
        self._step_lo = torch.from_numpy(np.tile(lo, self._graph_epochs)).to(dev)
        self._step_n = torch.from_numpy(np.tile(np.asarray(self._batch_lens, np.int32), self._graph_epochs)).to(dev)

    def _index_run(self, steps: int) -> None:
        """the index of a run's first `steps` steps from their staged draws"""
        ops.cvib_index(self.users_tensor, self.items_tensor, self._step_lo[:steps], self._step_n[:steps], self._draws[:steps],
                       self.model.user_num, self.model.item_num, out=self._index[:steps])


# ------------------------------------------------------------------------------------------------ own gradient passes
class _WholePassMixin(_SingleProcessMixin):
    """What the managers share whose gradient pass is ONE ops.*_grad call that is the whole step's loss (_OwnPassMixin,
    _DeviceDrawnMixin): the pass writes the reported loss terms, named by _LOSS_KEYS, into the first slots of the step's
    losses, and the engine's row-plan scratch is sized for the first two tables of the flat state."""
    _make_tables = staticmethod(lambda views: _capi.make_pure_tables(views[:2]))
    loss_dicts = _OuterLoop.__dict__['loss_dicts']      # the plain zip, in front of _BasicTrainManager's arithmetic


class _OwnPassMixin(_WholePassMixin):
    """A step whose gradient pass is the model's own (the MACR, LinearTrans-MF and CausE managers below), in front of a
    _BasicTrainManager.  Always the engine's unfused sequence: the own pass (one ops.*_grad call: every row of every gradient
    overwritten, the reported loss terms written into the first slots of the step's losses) -> the dense / ranged Adam over
    the whole flat state, which holds all the model's tensors.  The minibatches are static, so each one's inverted index
    (ops.macr_index) is built once on the host and kept on the device; the pass reads ids and index when it runs, and the
    ranged Adam launch carries the device-side schedule, so whole epochs replay as graphs.  Single process.

    A manager supplies: _SINGLE (the refusal's text), _LOSS_KEYS, _workspace_bytes(), _own_pass(), and, where a caller's
    minibatch can be one the step must refuse, _check_caller_batch()."""
    _lazy_adam_unsupported = "the model's own gradient pass stores zeros to every idle row: its cost follows the tables"

    def __init__(self, model, evaluator, device: torch.device, training_data: torch.Tensor, batch_size: int, epochs: int,
                 evaluate_interval: int, lr: float, L2_coe: float, L1_coe: float, test_begin_epoch: int = 0, *, rank=None,
                 world_size=None, process_group=None):
        self._require_single_process(world_size)
        super().__init__(model, evaluator, device, training_data, batch_size, epochs, evaluate_interval, lr, L2_coe, L1_coe,
                         test_begin_epoch, rank=rank, world_size=world_size, process_group=process_group)
        self._require_single_process(self.world_size)
        self._unfused = True        # gradient pass -> Adam, never the fused / alternating step
        self._index = None          # per static minibatch: (user_ptr, user_pos, item_ptr, item_pos) on the device
        self._caller = None         # train_a_batch: (users, items, index) of the caller's minibatch
        self._ws = ops.Workspace(self.device)
        self._ws.get(max(self._workspace_bytes(min(batch_size, self.n_total)), 16))   # sized once: capturable launches

    def _workspace_bytes(self, batch: int) -> int:
        """ops.*_workspace_bytes of the pass over a minibatch of `batch` rows"""
        raise NotImplementedError

    def _own_pass(self, users, items, scores, index, losses6: torch.Tensor) -> None:
        """the ops.*_grad call: the gradient of one minibatch into state.g_views, its loss terms into losses6's first slots"""
        raise NotImplementedError

    def _check_caller_batch(self, batch_users_tensor, batch_items_tensor) -> None:
        """raises on a caller's minibatch the step cannot take, before anything of it is kept"""

    def _raw_setup(self):
        super()._raw_setup()
        if self._index is None:
            u, v, m = self.users_tensor.cpu().numpy(), self.items_tensor.cpu().numpy(), self.model
            self._index = [ops.macr_index_device(u[b.lo:b.lo + b.n], v[b.lo:b.lo + b.n], m.user_num, m.item_num, self.device)
                           for b in self._raw_batches]

    def _gradient_pass(self, k, plan, users, items, envs, scores, weights, batch_norm: int, coefs, flags: int,
                       losses6: torch.Tensor, sched=None) -> None:
        if k is None:
            users, items, index = self._caller
        else:
            index = self._index[k]
        self._own_pass(users, items, scores, index, losses6)

    def train_a_batch(self, batch_users_tensor, batch_items_tensor, batch_scores_tensor, *args) -> dict:
        """train.py:379-405 / baseline_train.py:674-722 on caller tensors: this minibatch's index is built here, then one
        step."""
        self._check_caller_batch(batch_users_tensor, batch_items_tensor)
        dev, m = self.device, self.model
        ud = batch_users_tensor.detach().to(dev).reshape(-1).to(torch.int64).contiguous()
        vd = batch_items_tensor.detach().to(dev).reshape(-1).to(torch.int64).contiguous()
        self._caller = (ud, vd, ops.macr_index_device(ud, vd, m.user_num, m.item_num, dev))
        try:
            return self._batch_step(ud, vd, batch_scores_tensor, None, lambda: None)
        finally:
            self._caller = None


class _DeviceDrawnMixin(_RunIndexMixin, _WholePassMixin):
    """A step whose gradient pass is the model's own over the minibatch's rows and as many pairs drawn per step ON THE DEVICE
    (the BPR and doubly robust managers below), in front of a _BasicTrainManager.  Always the engine's unfused sequence: the
    pass (one ops.*_grad call: every row of every gradient overwritten) -> dense / ranged Adam; the pass is the whole step,
    so nothing stands between them (the engine's _after_gradient_pass as it is).

    `seed` names the trajectory and `step_id`, the global step counter, the next step's draws: together they key every draw,
    so the same seed gives the same bits whatever the run lengths, with graphs or without.  Before a run of epochs is enqueued
    its steps are named (step_id + 0, 1, ... into `_step_ids`), ONE draw launch fills their staging rows and ONE ops.cvib_index
    pass indexes them (_RunIndexMixin); step_id moves on by the steps actually issued.  A caller's minibatch
    (train_a_batch) is one step under the next step id.

    A manager supplies: _SINGLE, _LOSS_KEYS, _workspace_bytes(),
      _draw_run(steps)   the draw launch: the staging rows of a run's first `steps` steps, named _step_ids[:steps]
      _own_pass(users, items, scores, draws, index, weights, losses6)   the ops.*_grad call: the gradient of one step into
                         state.g_views, its loss terms into losses6's first slots; draws: the step's staging row as [2, B] (a
                         caller's step: what train_a_batch handed to _caller_step)
      _row_weights()     one fp32 weight per training row on the device, or None
    Its constructor validates its arguments and ends with _init_device_draws(); its train_a_batch draws and indexes the
    caller's step and ends with _caller_step()."""

    def _init_device_draws(self, seed) -> None:
        self.seed, self.step_id = int(seed), 0
        self._caller = None         # train_a_batch: (users, items, draws, index, weights) of the caller's minibatch
        self._init_run_index()
        self._init_staging(2 * self._cap)

    def _staging_resized(self, rows: int) -> None:
        super()._staging_resized(rows)
        self._step_ramp = torch.arange(rows, dtype=torch.int64, device=self.device)
        self._step_ids = torch.zeros(rows, dtype=torch.int64, device=self.device)

    def _stage_draws(self, n: int) -> None:
        steps = n * self.batch_num
        torch.add(self._step_ramp[:steps], self.step_id, out=self._step_ids[:steps])
        self._draw_run(steps)
        self._index_run(steps)

    def _draws_consumed(self, steps: int) -> None:
        self.step_id += steps

    def _gradient_pass(self, k, plan, users, items, envs, scores, weights, batch_norm: int, coefs, flags: int,
                       losses6: torch.Tensor, sched=None) -> None:
        if k is None:
            users, items, draws, index, w = self._caller
        else:
            b, s = self._raw_batches[k], self._loss_slot * self.batch_num + k
            draws, index, w = self._draws[s, :, :b.n], self._index[s], self._row_weights()
            w = None if w is None else w[b.lo:b.lo + b.n]
        self._own_pass(users, items, scores, draws, index, w, losses6)

    def _step_name(self, B: int):
        """(step_n, step_id) of a caller's step of B rows, as the draw launches take them"""
        return (torch.full((1,), B, dtype=torch.int32, device=self.device),
                torch.full((1,), self.step_id, dtype=torch.int64, device=self.device))

    def _caller_step(self, users, items, scores, draws, index, weights) -> dict:
        """one step on a caller's minibatch whose draws were made under step_id"""
        self._ws.get(max(self._workspace_bytes(users.numel()), 16))
        self._caller = (users, items, draws, index, weights)
        try:
            out = self._batch_step(users, items, scores, None, lambda: None)
        finally:
            self._caller = None
        self.step_id += 1
        return out


# ------------------------------------------------------------------------------------------------ WMF
def wmf_distinct(users: np.ndarray, items: np.ndarray, batch_size: int) -> list:
    """per static minibatch of utils.mini_batch (unshuffled slices) the ascending distinct users and items, as torch.unique
    gives them (baseline_train.py:192-193): [(uu, ui), ...]"""
    users, items = np.asarray(users).reshape(-1), np.asarray(items).reshape(-1)
    return [(np.unique(users[lo:lo + batch_size]), np.unique(items[lo:lo + batch_size]))
            for lo in range(0, len(users), batch_size)]


def wmf_draw(uu: np.ndarray, ui: np.ndarray, user_batch_size: int, item_batch_size: int):
    """one step's selection (baseline_train.py:195-202): two np.random.shuffle calls on numpy's GLOBAL generator, users first,
    each permutation cut to its batch size and mapped through the distinct ids.  Host only."""
    ru = np.arange(len(uu))
    np.random.shuffle(ru)
    ri = np.arange(len(ui))
    np.random.shuffle(ri)
    return uu[ru[:user_batch_size]], ui[ri[:item_batch_size]]


def wmf_draw_epochs(distinct: list, user_batch_size: int, item_batch_size: int, epochs: int) -> list:
    """the selections of `epochs` whole epochs in the reference's order (step by step, users then items): [(Su, Si), ...]"""
    return [wmf_draw(uu, ui, user_batch_size, item_batch_size) for _ in range(epochs) for uu, ui in distinct]


class WMFTrainManager(_DrawnTermMixin, BasicImplicitTrainManager):
    """reference baseline_train.py:157-228: the PureMF step plus imputation_coe * BCE(sigmoid(Pu[a] . Qi[b]), 0) averaged over
    a block Su x Si drawn per step from the minibatch's distinct users and items (target 0, as the reference's `zero_tensor`
    is named -- the reference allocates it uninitialised).

    The term is torch.ops.invpref.impute_grad_ (csrc/invpref_impute.hip) on the drawn-term step of _DrawnTermMixin; nothing of
    the block is materialised.  A step's draw: two np.random.shuffle permutations of the minibatch's distinct users and items
    (listed once), users first, each cut to its batch size.

    selections= (keyword-only) is the mixin's draw source: a callable (uu, ui, user_batch_size, item_batch_size) -> (Su, Si),
    or an iterable of (Su, Si) pairs.  A step's Su / Si must hold min(distinct, batch size) ids of the minibatch."""
    _SINGLE = 'WMF runs in a single process (a sharded form would all-reduce the summed gradient before the imputation ' \
              'term is added; not implemented)'
    _WHAT = 'selection'
    _draw_default = staticmethod(wmf_draw)

    def __init__(self, model, evaluator, device, training_data: torch.Tensor, batch_size: int, epochs: int,
                 evaluate_interval: int, lr: float, L2_coe: float, L1_coe: float, test_begin_epoch: int = 0,
                 imputation_coe: float = 1.0, user_batch_size: int = 1000, item_batch_size: int = 1000, *, selections=None,
                 rank=None, world_size=None, process_group=None):
        if int(user_batch_size) < 1 or int(item_batch_size) < 1:
            raise ValueError('user_batch_size and item_batch_size must be at least 1')
        self._require_single_process(world_size)
        super().__init__(model, evaluator, device, training_data, batch_size, epochs, evaluate_interval, lr, L2_coe, L1_coe,
                         test_begin_epoch, rank=rank, world_size=world_size, process_group=process_group)
        self.imputation_coe = float(imputation_coe)
        self.user_batch_size, self.item_batch_size = int(user_batch_size), int(item_batch_size)
        distinct = wmf_distinct(self.users_tensor.cpu().numpy(), self.items_tensor.cpu().numpy(), batch_size)
        self._counts = [self._count(uu, ui) for uu, ui in distinct]
        self._cap_u = max(c[0] for c in self._counts)
        self._cap_i = max(c[1] for c in self._counts)
        self._init_draws(selections, [((uu, ui, self.user_batch_size, self.item_batch_size), c)
                                      for (uu, ui), c in zip(distinct, self._counts)], self._cap_u, self._cap_u + self._cap_i)
        self._imp_ws = ops.Workspace(self.device)
        self._imp_ws.get(max(ops.impute_workspace_bytes(max(self._cap_u, self.user_batch_size), self._cap_i,
                                                        model.factor_num), 8))   # sized once: capturable launches

    def _count(self, uu, ui):
        return min(len(uu), self.user_batch_size), min(len(ui), self.item_batch_size)

    def _impute(self, su, si, loss):
        st = self.state
        ops.impute_grad_(st.p_views[0], st.p_views[1], su, si, self.imputation_coe, st.g_views[0], st.g_views[1], loss, None,
                         self._imp_ws)

    def _term(self, k: int, s: int, loss: torch.Tensor) -> None:
        row = self._staged[s]
        nu, ni = self._counts[k]
        self._impute(row[:nu], row[self._cap_u:self._cap_u + ni], loss)

    def train_a_batch(self, batch_users_tensor, batch_items_tensor, batch_scores_tensor, *args) -> dict:
        """baseline_train.py:179-228 on caller tensors: the distinct ids of THIS batch, two draws, one step."""
        u = batch_users_tensor.detach().cpu().numpy().reshape(-1)
        v = batch_items_tensor.detach().cpu().numpy().reshape(-1)
        uu, ui = np.unique(u), np.unique(v)
        su, si = self._draw((uu, ui, self.user_batch_size, self.item_batch_size), self._count(uu, ui))
        return self._batch_step(u, v, batch_scores_tensor, None, lambda: self._impute(
            torch.from_numpy(su).to(self.device), torch.from_numpy(si).to(self.device), self.state.losses6[5:6]))


# ------------------------------------------------------------------------------------------------ CVIB-MF
def cvib_draw(user_num: int, item_num: int, n: int):
    """one step's drawn pairs (baseline_train.py:617-620 / :1013-1016): two np.random.randint calls on numpy's GLOBAL
    generator, users first.  Host only."""
    ru = np.random.randint(0, user_num, n)
    rv = np.random.randint(0, item_num, n)
    return ru, rv


def cvib_draw_epochs(user_num: int, item_num: int, batch_lens, epochs: int) -> list:
    """the drawn pairs of `epochs` whole epochs in the reference's order (step by step, as many pairs as the minibatch has
    rows): [(ru, rv), ...]"""
    return [cvib_draw(user_num, item_num, n) for _ in range(epochs) for n in batch_lens]


class _CVIBMixin(_RunIndexMixin, _DrawnTermMixin):
    """CVIBTrainManager / CVIBExplicitTrainManager (baseline_train.py:584-647, :978-1044): the PureMF step plus
    info_coe * info, info = alpha * (-pbar log qbar - (1 - pbar) log(1 - qbar)) + gamma * mean(p log p), p the predictions at
    the minibatch's pairs, qbar the mean prediction at as many uniformly drawn (user, item) pairs (the explicit form clips the
    logarithms' arguments at eps).  `info` is visible inside 'loss' only.

    The term is torch.ops.invpref.cvib_grad_ (csrc/invpref_cvib.hip: means, fold, scatter, boundary) on the drawn-term step of
    _DrawnTermMixin.  A step's draw: np.random.randint, users then items, B = the minibatch's rows.  Behind the copy of a
    run's draws they are indexed on the device (_RunIndexMixin).

    draws= (keyword-only) is the mixin's draw source: a callable (user_num, item_num, n) -> (ru, rv), or an iterable of
    (ru, rv) pairs."""
    _SINGLE = 'CVIB runs in a single process (a sharded form would all-reduce the two means and the summed gradient; ' \
              'not implemented)'
    _WHAT = 'draw'
    _draw_default = staticmethod(cvib_draw)

    def _cvib_init(self, alpha, gamma, info_coe, eps, draws):
        # (the engine's `alpha` is what _alpha_for() hands to _coefs(), which a PureMF step never reads: the attribute is CVIB's
        #  here, as in the reference)
        self.alpha, self.gamma, self.info_coe, self.eps = float(alpha), float(gamma), float(info_coe), float(eps)
        self._init_run_index()
        self._init_draws(draws, [((self.model.user_num, self.model.item_num, b), (b, b)) for b in self._batch_lens],
                         self._cap, 2 * self._cap)

    def _workspace_bytes(self, batch: int) -> int:
        return ops.cvib_workspace_bytes(batch, self.model.factor_num)

    def _after_staging(self, steps: int) -> None:
        self._index_run(steps)

    def _info_term(self, users, items, draw_users, draw_items, index, loss_slot):
        st = self.state
        ops.cvib_grad_(st.p_views[0], st.p_views[1], users, items, draw_users, draw_items, index, self.implicit, self.alpha,
                       self.gamma, self.info_coe, self.eps, st.g_views[0], st.g_views[1], loss_slot, None, None, None,
                       self._ws)

    def _term(self, k: int, s: int, loss: torch.Tensor) -> None:
        b = self._raw_batches[k]
        self._info_term(b.users, b.items, self._draws[s, 0, :b.n], self._draws[s, 1, :b.n], self._index[s], loss)

    def train_a_batch(self, batch_users_tensor, batch_items_tensor, batch_scores_tensor, *args) -> dict:
        """baseline_train.py:606-647 / :1002-1044 on caller tensors: as many drawn pairs as the batch has rows, one step."""
        u = batch_users_tensor.detach().cpu().numpy().reshape(-1)
        v = batch_items_tensor.detach().cpu().numpy().reshape(-1)
        ru, rv = self._draw((self.model.user_num, self.model.item_num, len(u)), (len(u), len(u)))
        dev = self.device
        ud = torch.from_numpy(np.ascontiguousarray(u, dtype=np.int64)).to(dev)
        vd = torch.from_numpy(np.ascontiguousarray(v, dtype=np.int64)).to(dev)
        rud, rvd = torch.from_numpy(np.stack([ru, rv])).to(dev)
        index = ops.step_index(ud, vd, rud, rvd, self.model.user_num, self.model.item_num)
        self._ws.get(max(self._workspace_bytes(len(u)), 16))
        return self._batch_step(u, v, batch_scores_tensor, None, lambda: self._info_term(
            ud, vd, rud, rvd, index, self.state.losses6[5:6]))


class CVIBTrainManager(_CVIBMixin, BasicImplicitTrainManager):
    """reference baseline_train.py:584-647 (BCELoss + the information term; no clip)"""

    def __init__(self, model, evaluator, device, training_data: torch.Tensor, batch_size: int, epochs: int,
                 evaluate_interval: int, lr: float, L2_coe: float, L1_coe: float, test_begin_epoch: int = 0,
                 alpha: float = 0.1, gamma: float = 0.01, info_coe: float = 1.0, *, draws=None, rank=None, world_size=None,
                 process_group=None):
        self._require_single_process(world_size)
        super().__init__(model, evaluator, device, training_data, batch_size, epochs, evaluate_interval, lr, L2_coe, L1_coe,
                         test_begin_epoch, rank=rank, world_size=world_size, process_group=process_group)
        self._cvib_init(alpha, gamma, info_coe, 0.0, draws)


class CVIBExplicitTrainManager(_CVIBMixin, BasicExplicitTrainManager):
    """reference baseline_train.py:978-1044 (MSELoss + the information term, logarithms clipped at eps)"""

    def __init__(self, model, evaluator, device, training_data: torch.Tensor, batch_size: int, epochs: int,
                 evaluate_interval: int, lr: float, L2_coe: float, L1_coe: float, test_begin_epoch: int = 0,
                 alpha: float = 0.1, gamma: float = 0.01, info_coe: float = 1.0, eps: float = 1e-1, *, draws=None, rank=None,
                 world_size=None, process_group=None):
        self._require_single_process(world_size)
        super().__init__(model, evaluator, device, training_data, batch_size, epochs, evaluate_interval, lr, L2_coe, L1_coe,
                         test_begin_epoch, rank=rank, world_size=world_size, process_group=process_group)
        self._cvib_init(alpha, gamma, info_coe, eps, draws)


# ------------------------------------------------------------------------------------------------ fairness-MF
def fairness_item_table(items, item_num: int, weight_smooth_coe: float):
    """(counts int32 [item_num], table float32 [range + 1]) of init_item_distance (baseline_train.py:251-277): the reference's
    item_num x item_num matrix is a function of |cnt_x - cnt_y| alone, S[x][y] == table[|counts[x] - counts[y]|] bit for bit
    (float64 (d / range) ** w, then float32; 0 ** 0 = 1 at w = 0).  counts = bincount(minlength=item_num): the reference's own
    whenever the largest item id occurs in training (where it does not, the reference's draw indexes past its matrix and
    raises).  Equal counts everywhere: ValueError (the reference divides 0 by 0)."""
    items = np.asarray(items).reshape(-1).astype(np.int64)
    if len(items) == 0 or items.min() < 0 or items.max() >= item_num:
        raise ValueError(f'item ids must lie in [0, {item_num})')
    counts = np.bincount(items, minlength=int(item_num))
    span = int(counts.max() - counts.min())
    if span == 0:
        raise ValueError('every item has the same number of training rows: the distance |cnt_x - cnt_y| / (max - min) is 0 / 0')
    table = ((np.arange(span + 1, dtype=np.float64) / float(span)) ** float(weight_smooth_coe)).astype(np.float32)
    return counts.astype(np.int32), table


def fairness_draw(item_num: int, n: int) -> np.ndarray:
    """one step's drawn items (baseline_train.py:291): one np.random.randint call on numpy's GLOBAL generator, WITH
    replacement.  Host only."""
    return np.random.randint(0, item_num, size=n)


def fairness_draw_epochs(item_num: int, n: int, batch_num: int, epochs: int) -> list:
    """the draws of `epochs` whole epochs of batch_num steps in the reference's order: [idx, ...]"""
    return [fairness_draw(item_num, n) for _ in range(epochs * batch_num)]


class FairnessMFTrainManager(_DrawnTermMixin, BasicImplicitTrainManager):
    """reference baseline_train.py:231-313: the PureMF step plus fairness_coe * trace(R S R^T) / B, R = the predictions of the
    minibatch's users (one row per interaction) at item_batch_size items drawn per step with replacement, S the items'
    popularity distance (|cnt_x - cnt_y| / (max cnt - min cnt)) ** weight_smooth_coe.  The term is visible inside 'loss' only.

    The term is torch.ops.invpref.fairness_grad_ (csrc/invpref_fairness.hip) on the drawn-term step of _DrawnTermMixin.  Rows of
    one user are identical, so a minibatch is its distinct users with their multiplicities (listed once per static minibatch);
    S is never built: the kernel forms it from the per-item counts and the 1-D table of fairness_item_table().  Neither a
    [B, item_num] prediction matrix nor an item_num x item_num matrix exists, on the device or the host.

    draws= (keyword-only) is the mixin's draw source: a callable (item_num, n) -> ids, or an iterable of recorded draws."""
    _SINGLE = 'fairness-MF runs in a single process (a sharded form would all-reduce the summed gradient before the fairness ' \
              'term is added; not implemented)'
    _WHAT = 'draw'
    _ONE_ARRAY = True
    _draw_default = staticmethod(fairness_draw)

    def __init__(self, model, evaluator, device, training_data: torch.Tensor, batch_size: int, epochs: int,
                 evaluate_interval: int, lr: float, L2_coe: float, L1_coe: float, test_begin_epoch: int = 0,
                 fairness_coe: float = 1.0, weight_smooth_coe: float = 1.0, item_batch_size: int = 1000, *, draws=None,
                 rank=None, world_size=None, process_group=None):
        if int(item_batch_size) < 1:
            raise ValueError('item_batch_size must be at least 1')
        self._require_single_process(world_size)
        super().__init__(model, evaluator, device, training_data, batch_size, epochs, evaluate_interval, lr, L2_coe, L1_coe,
                         test_begin_epoch, rank=rank, world_size=world_size, process_group=process_group)
        self.fairness_coe, self.weight_smooth_coe = float(fairness_coe), float(weight_smooth_coe)
        self.item_batch_size = J = int(item_batch_size)
        counts, table = fairness_item_table(self.items_tensor.cpu().numpy(), model.item_num, weight_smooth_coe)
        self.item_counts = torch.from_numpy(counts).to(self.device)
        self.item_distance_table = torch.from_numpy(table).to(self.device)
        users = self.users_tensor.cpu().numpy().reshape(-1)
        self._users = [self._distinct(users[lo:lo + batch_size]) for lo in range(0, len(users), batch_size)]
        self._init_draws(draws, [((model.item_num, J), (J, 0))] * len(self._users), J, J)
        self._fair_ws = ops.Workspace(self.device)
        self._fair_ws.get(max(ops.fairness_workspace_bytes(max(len(u) for u, _, _ in self._users), J, model.factor_num),
                              16))   # sized once: capturable launches

    def _distinct(self, users: np.ndarray):
        """(distinct users, their multiplicities, rows) of one minibatch, int32 on the device"""
        uu, m = np.unique(users, return_counts=True)
        return (torch.from_numpy(uu.astype(np.int32)).to(self.device), torch.from_numpy(m.astype(np.int32)).to(self.device),
                len(users))

    def _fairness(self, users, mult, rows, idx, loss):
        st = self.state
        ops.fairness_grad_(st.p_views[0], st.p_views[1], users, mult, idx, self.item_counts, self.item_distance_table,
                           self.fairness_coe, rows, st.g_views[0], st.g_views[1], loss, None, self._fair_ws)

    def _term(self, k: int, s: int, loss: torch.Tensor) -> None:
        self._fairness(*self._users[k], self._staged[s], loss)

    def train_a_batch(self, batch_users_tensor, batch_items_tensor, batch_scores_tensor, *args) -> dict:
        """baseline_train.py:279-313 on caller tensors: the distinct users of THIS batch, one draw, one step."""
        u = batch_users_tensor.detach().cpu().numpy().reshape(-1)
        v = batch_items_tensor.detach().cpu().numpy().reshape(-1)
        idx, _ = self._draw((self.model.item_num, self.item_batch_size), (self.item_batch_size, 0))
        uu, m, rows = self._distinct(u)
        return self._batch_step(u, v, batch_scores_tensor, None, lambda: self._fairness(
            uu, m, rows, torch.from_numpy(idx).to(self.device), self.state.losses6[5:6]))


# ------------------------------------------------------------------------------------------------ MACR-MF
class LinearImplicitScorePredictor(nn.Module):
    """models.py:223-246: sigmoid(linear_map(x)), the weight xavier-uniform, the bias nn.Linear's default"""

    def __init__(self, factor_dim: int):
        super().__init__()
        self.linear_map = nn.Linear(factor_dim, 1)
        self.output_func = nn.Sigmoid()
        nn.init.xavier_uniform_(self.linear_map.weight)
        self.elements_num = float(factor_dim)

    def forward(self, invariant_preferences):
        """one value per row, on the device kernel of the MACR pass (values only: training goes through MACR's forward)"""
        x = invariant_preferences.detach().float().contiguous()
        return ops.macr_branch(x.reshape(-1, x.shape[-1]), self.linear_map.weight.detach(),
                               self.linear_map.bias.detach()).reshape(*x.shape[:-1], 1)


class _OwnPassLoss(torch.autograd.Function):
    """score_loss of a model's forward through its own gradient pass (MACR-MF, LinearTrans-MF): the pass forms the loss and the
    gradients of all the model's tensors at once, backward() scales them by the upstream scalar.  grad_pass(data, grads, users,
    items, scores, index, losses4): the model's ops.*_grad call with its coefficients and L2_coe = L1_coe = 0."""

    @staticmethod
    def forward(ctx, grad_pass, users, items, scores, *tables):
        data = [t.detach().contiguous() for t in tables]
        dev = data[0].device
        users, items = users.reshape(-1).long().contiguous(), items.reshape(-1).long().contiguous()
        index = ops.macr_index_device(users, items, data[0].shape[0], data[1].shape[0], dev)
        grads = [torch.empty_like(t) for t in data]
        losses = torch.empty(4, dtype=torch.float32, device=dev)
        grad_pass(data, grads, users, items, scores.detach().reshape(-1).float().contiguous(), index, losses)
        ctx.save_for_backward(*grads)
        return losses[0].clone()

    @staticmethod
    def backward(ctx, gs):
        scale = gs.detach().to(torch.float32)
        return (None, None, None, None, *[g * scale for g in ctx.saved_tensors])


def _user_ids(users_id, table: torch.Tensor) -> torch.Tensor:
    """users_id as flat, contiguous int64 on the table's device"""
    return torch.as_tensor(users_id).to(table.device).reshape(-1).to(torch.int64).contiguous()


class MACRMatrixFactorization(nn.Module):
    """baseline_models.py:139-234: MF whose training score is sigmoid(u . i) * sigmoid(wu . u + bu) * sigmoid(wi . i + bi) --
    the interaction, user and item branches -- and whose ranking score is the counterfactual
    (sigmoid(u . i) - const_c) * user branch * item branch.  The reference's constructor order (the same torch.manual_seed
    gives the same initial state_dict), parameter and attribute names.

    Not a PureMatrixFactorization: ImplicitTestManager never ranks it by sigmoid(u . i) alone but by rank_fn(), the scaled scan
    of csrc/invpref_retrieve.hip (its topk() keeps the predict() + top-k route of any other model).  forward / predict run on
    csrc/invpref_macr.hip; forward builds the minibatch's inverted index
    on the host per call (the unfused surface -- MACRTrainManager prepares it once per static minibatch)."""
    implicit = True

    def __init__(self, user_num: int, item_num: int, factor_num: int, const_c: float, item_coe: float, user_coe: float):
        super().__init__()
        self.user_num, self.item_num, self.factor_num = user_num, item_num, factor_num
        self.user_emb = nn.Embedding(user_num, factor_num)
        self.item_emb = nn.Embedding(item_num, factor_num)
        self.output_func = nn.Sigmoid()
        self.const_c = const_c
        self.user_predictor = LinearImplicitScorePredictor(factor_num)
        self.item_predictor = LinearImplicitScorePredictor(factor_num)
        self.loss_func = nn.BCELoss()
        self.item_coe, self.user_coe = item_coe, user_coe
        nn.init.normal_(self.user_emb.weight, std=0.01)  # baseline_models.py:160-162
        nn.init.normal_(self.item_emb.weight, std=0.01)
        self._absent = None

    def tables(self):
        """the six parameters in state_dict order"""
        return [self.user_emb.weight, self.item_emb.weight, self.user_predictor.linear_map.weight,
                self.user_predictor.linear_map.bias, self.item_predictor.linear_map.weight, self.item_predictor.linear_map.bias]

    def forward(self, users_id, items_id, ground_truth):  # baseline_models.py:164-182: the three-branch score loss
        uc, ic = float(self.user_coe), float(self.item_coe)
        return _OwnPassLoss.apply(lambda data, grads, u, v, y, index, losses: ops.macr_grad(
            data, grads, u, v, y, index, uc, ic, 0., 0., losses), users_id, items_id, ground_truth, *self.tables())

    # PureMF's regularisers over the gathered embedding rows (baseline_models.py:184-208; the predictors are not covered)
    _seven = _PureMFBase._seven
    _reg = _PureMFBase._reg
    get_L1_reg = _PureMFBase.get_L1_reg
    get_L2_reg = _PureMFBase.get_L2_reg

    def branches(self):
        """(user branch [user_num], item branch [item_num]): sigmoid(w . row + b) of every row"""
        up, ip = self.user_predictor.linear_map, self.item_predictor.linear_map
        return (ops.macr_branch(self.user_emb.weight.detach(), up.weight.detach(), up.bias.detach()),
                ops.macr_branch(self.item_emb.weight.detach(), ip.weight.detach(), ip.bias.detach()))

    def predict(self, users_id):  # baseline_models.py:210-234
        a, c = self.branches()
        return ops.macr_predict(self.user_emb.weight.detach(), self.item_emb.weight.detach(),
                                _user_ids(users_id, self.user_emb.weight), a, c, self.const_c)

    def rank_fn(self):
        """ImplicitTestManager's fused route: f(users, k, mask, highlight, truth) -> (items, scores, hits) ranking by the
        scores of predict() without their matrix -- the two branch launches here, then one scaled scan per call of f"""
        a, c = self.branches()
        P, Q = self.user_emb.weight.detach().contiguous(), self.item_emb.weight.detach().contiguous()
        return lambda users, k, mask, highlight, truth: ops.predict_topk_scaled(
            P, Q, users, k, a, c, self.const_c, True, mask=mask, highlight=highlight, truth=truth)

    def truth_rank_fn(self):
        """ImplicitRankTestManager's fused route, the counterpart of rank_fn(): f(users, truth, mask, highlight) -> int32 ranks
        of the truth items in the ranking by the scores of predict(), without their matrix -- the two branch launches here,
        then one scaled rank scan per call of f.  Nothing is kept between calls of truth_rank_fn()"""
        a, c = self.branches()
        P, Q = self.user_emb.weight.detach().contiguous(), self.item_emb.weight.detach().contiguous()
        return lambda users, truth, mask, highlight: ops.truth_ranks_scaled(
            P, Q, users, truth, a, c, self.const_c, True, mask=mask, highlight=highlight)

    def recommend(self, users_id, k: int, exclude=None, highlight=None):
        """Each user's top-k items by the scores of predict() (which may be negative), `exclude` items scoring -1024 and
        `highlight` items += 1024 (CSR pairs aligned with users_id): the branches once, then the scaled scan
        (ops.predict_topk_scaled with shift = const_c) -- no rating matrix; the ranking of predict()'s matrix item for item
        and score for score.  -> (items int64[n, k], scores fp32[n, k])"""
        a, c = self.branches()
        users = torch.as_tensor(users_id).to(self.user_emb.weight.device)
        return ops.recommend(self.user_emb.weight, self.item_emb.weight, users, k, exclude=exclude, highlight=highlight,
                             user_scale=a, item_scale=c, shift=self.const_c)


class MACRTrainManager(_OwnPassMixin, BasicImplicitTrainManager):
    """MACR (baseline/special_bias/macr_mf_main.py) under the reference's plain BasicImplicitTrainManager (train.py:345-461):
    loss = model(users, items, scores) + L2_coe * L2_reg + L1_coe * L1_reg, Adam over all six tensors.  The own-pass step of
    _OwnPassMixin on ops.macr_grad (csrc/invpref_macr.hip)."""
    _SINGLE = 'MACR runs in a single process (a sharded form would all-reduce the gradients of all six tensors; not implemented)'

    def _workspace_bytes(self, batch: int) -> int:
        m = self.model
        return ops.macr_workspace_bytes(m.user_num, m.item_num, batch, m.factor_num)

    def _own_pass(self, users, items, scores, index, losses6: torch.Tensor) -> None:
        st, m = self.state, self.model
        ops.macr_grad(st.p_views, st.g_views, users, items, scores, index, m.user_coe, m.item_coe, self.L2_coe, self.L1_coe,
                      losses6[:4], self._ws)


# ------------------------------------------------------------------------------------------------ LinearTrans-MF
class LinearTransMatrixFactorization(nn.Module):
    """baseline_models.py:72-136: MF whose score is sigmoid(w . (u (*) i) + b) -- InvPref's LinearImplicitScorePredictor over the
    element-wise product of ONE pair of tables: the single-branch ablation of InvPref, trained with its predictor under the plain
    BasicImplicitTrainManager.  The reference's constructor order (the same torch.manual_seed gives the same initial
    state_dict), parameter and attribute names.

    Not a PureMatrixFactorization: ImplicitTestManager ranks it by rank_fn(), the weighted scan of csrc/invpref_retrieve.hip
    (its topk() keeps the predict() + top-k route of any other model).  forward / predict run on csrc/invpref_lintrans.hip;
    predict() never builds the reference's [n item_num, D] temporary.  forward builds the minibatch's inverted index on the
    host per call (the unfused surface -- LinearTransTrainManager prepares it once per static minibatch)."""
    implicit = True

    def __init__(self, user_num: int, item_num: int, factor_num: int):
        super().__init__()
        self.user_num, self.item_num, self.factor_num = user_num, item_num, factor_num
        self.user_emb = nn.Embedding(user_num, factor_num)
        self.item_emb = nn.Embedding(item_num, factor_num)
        self.linear_predictor = LinearImplicitScorePredictor(factor_num)
        self.loss_func = nn.BCELoss()
        nn.init.normal_(self.user_emb.weight, std=0.01)  # baseline_models.py:83-85
        nn.init.normal_(self.item_emb.weight, std=0.01)
        self._absent = None

    def tables(self):
        """the four parameters in state_dict order"""
        return [self.user_emb.weight, self.item_emb.weight, self.linear_predictor.linear_map.weight,
                self.linear_predictor.linear_map.bias]

    def forward(self, users_id, items_id, ground_truth):  # baseline_models.py:87-93: the score loss
        return _OwnPassLoss.apply(lambda data, grads, u, v, y, index, losses: ops.lintrans_grad(
            data, grads, u, v, y, index, 0., 0., losses), users_id, items_id, ground_truth, *self.tables())

    # PureMF's regularisers over the gathered embedding rows plus the predictor's own terms (baseline_models.py:95-119,
    # models.py:237-243) -- D + 1 numbers, summed by torch as the reference does; the training pass has them in its kernels
    _seven = _PureMFBase._seven
    _reg = _PureMFBase._reg

    def get_L1_reg(self, users_id, items_id):
        lm = self.linear_predictor.linear_map
        return self._reg(users_id, items_id, 1) + torch.norm(lm.weight, 1) / float(self.factor_num) + torch.norm(lm.bias, 1)

    def get_L2_reg(self, users_id, items_id):
        lm = self.linear_predictor.linear_map
        return (self._reg(users_id, items_id, 2) + torch.norm(lm.weight, 2).pow(2) / float(self.factor_num)
                + torch.norm(lm.bias, 2).pow(2))

    def _frozen(self):
        """(user table, item table, weight [D], bias [1]) detached and contiguous"""
        lm = self.linear_predictor.linear_map
        return (self.user_emb.weight.detach().contiguous(), self.item_emb.weight.detach().contiguous(),
                lm.weight.detach().reshape(-1).contiguous(), lm.bias.detach().contiguous())

    def predict(self, users_id):  # baseline_models.py:121-136
        P, Q, w, b = self._frozen()
        return ops.lintrans_predict(P, Q, _user_ids(users_id, P), w, b)

    def rank_fn(self):
        """ImplicitTestManager's fused route: f(users, k, mask, highlight, truth) -> (items, scores, hits) ranking by the
        scores of predict() without their matrix -- one weighted scan per call of f; weight and bias stay on the device, so a
        captured evaluation follows them"""
        P, Q, w, b = self._frozen()
        return lambda users, k, mask, highlight, truth: ops.predict_topk_weighted(
            P, Q, users, k, w, b, True, mask=mask, highlight=highlight, truth=truth)

    def truth_rank_fn(self):
        """ImplicitRankTestManager's fused route, the counterpart of rank_fn(): f(users, truth, mask, highlight) -> int32 ranks
        of the truth items in the ranking by the scores of predict(), without their matrix -- one weighted rank scan per call
        of f; weight and bias stay on the device, so a captured evaluation follows them"""
        P, Q, w, b = self._frozen()
        return lambda users, truth, mask, highlight: ops.truth_ranks_weighted(
            P, Q, users, truth, w, b, True, mask=mask, highlight=highlight)

    def recommend(self, users_id, k: int, exclude=None, highlight=None):
        """Each user's top-k items by the scores of predict(), `exclude` items scoring -1024 and `highlight` items += 1024
        (CSR pairs aligned with users_id): the weighted scan (ops.predict_topk_weighted) -- no rating matrix; the ranking of
        predict()'s matrix item for item and score for score.  -> (items int64[n, k], scores fp32[n, k])"""
        P, Q, w, b = self._frozen()
        users = torch.as_tensor(users_id).to(P.device)
        return ops.recommend(P, Q, users, k, exclude=exclude, highlight=highlight, dim_weight=w, logit_bias=b)


class LinearTransTrainManager(_OwnPassMixin, BasicImplicitTrainManager):
    """LinearTrans-MF under the reference's plain BasicImplicitTrainManager (train.py:345-461):
    loss = model(users, items, scores) + L2_coe * L2_reg + L1_coe * L1_reg with the predictor inside both regularisers, Adam over
    all four tensors.  The own-pass step of _OwnPassMixin on ops.lintrans_grad (csrc/invpref_lintrans.hip)."""
    _SINGLE = ('LinearTrans-MF runs in a single process (a sharded form would all-reduce the gradients of all four tensors; '
               'not implemented)')

    def _workspace_bytes(self, batch: int) -> int:
        m = self.model
        return ops.lintrans_workspace_bytes(m.user_num, m.item_num, batch, m.factor_num)

    def _own_pass(self, users, items, scores, index, losses6: torch.Tensor) -> None:
        st = self.state
        ops.lintrans_grad(st.p_views, st.g_views, users, items, scores, index, self.L2_coe, self.L1_coe, losses6[:4], self._ws)


# ------------------------------------------------------------------------------------------------ CausE
CAUSE_LOSS_KEYS = ['train_score_loss', 'uniform_score_loss', 'teacher_reg', 'L2_reg', 'loss']  # baseline_train.py:715-721


class _CausEModelMixin:
    """What CausEMatrixFactorization and its explicit twin share (baseline_models.py:555-649, :706-794): a student pair and a
    teacher pair of tables, created and re-drawn in the reference's order (user_emb, item_emb, teacher_user_emb,
    teacher_item_emb: the same torch.manual_seed gives the same state_dict), and the reference's methods with their
    `train_teacher` switch on the unfused forward / regulariser functions, applied to the chosen pair."""

    def __init__(self, user_num: int, item_num: int, factor_num: int):
        nn.Module.__init__(self)
        self.user_num, self.item_num, self.factor_num = user_num, item_num, factor_num
        self.user_emb = nn.Embedding(user_num, factor_num)
        self.item_emb = nn.Embedding(item_num, factor_num)
        self.teacher_user_emb = nn.Embedding(user_num, factor_num)
        self.teacher_item_emb = nn.Embedding(item_num, factor_num)
        if self.implicit:
            self.output_func = nn.Sigmoid()
            self.loss_func = nn.BCELoss()
        else:
            self.loss_func = nn.MSELoss()
        for emb in (self.user_emb, self.item_emb, self.teacher_user_emb, self.teacher_item_emb):
            nn.init.normal_(emb.weight, std=0.01)
        self._absent = None

    def tables(self):
        """the four tables in state_dict order: the student's first, so whatever ranks tables()[0] . tables()[1] ranks the
        student"""
        return [self.user_emb.weight, self.item_emb.weight, self.teacher_user_emb.weight, self.teacher_item_emb.weight]

    def _pair(self, train_teacher: bool):
        return ((self.teacher_user_emb.weight, self.teacher_item_emb.weight) if train_teacher
                else (self.user_emb.weight, self.item_emb.weight))

    def _stand_ins(self, rows_user: int, rows_item: int):
        w = self.user_emb.weight
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=w.device)  # noqa: E731
        D = self.factor_num
        return [z(rows_user, D), z(rows_item, D), z(1, D), z(1, D), z(1)]

    def _seven(self, train_teacher: bool = False):
        w = self.user_emb.weight
        if self._absent is None or self._absent[0].device != w.device:
            self._absent = self._stand_ins(self.user_num, self.item_num)
        return list(self._pair(train_teacher)) + self._absent

    def _scores(self, users_id, items_id, train_teacher: bool = False):
        from .autograd import InvPrefForward
        inv, _, _ = InvPrefForward.apply(users_id, items_id, torch.zeros_like(users_id), 0., self.implicit,
                                         *self._seven(train_teacher))
        return inv

    def forward(self, users_id, items_id, train_teacher, ground_truth=None):  # baseline_models.py:574-593 / :724-742
        final_ratings = self._scores(users_id, items_id, bool(train_teacher)).reshape(-1)
        if ground_truth is not None:
            return self.loss_func(final_ratings, ground_truth)
        return final_ratings

    def _reg(self, users_id, items_id, norm: int, train_teacher: bool = False):
        from .autograd import InvPrefReg
        if not self.implicit:
            return 2. * InvPrefReg.apply(users_id, items_id, torch.zeros_like(users_id), norm, True, False,
                                         *self._seven(train_teacher))
        # baseline_models.py:608-619: the implicit model's get_items_reg gathers the USER table of the chosen pair with the
        # ITEM ids -- the regulariser runs over (user table, user table), and an item id beyond it is the reference's IndexError
        if items_id.numel() and int(items_id.max()) >= self.user_num:
            raise IndexError(f'index out of range in self: item id {int(items_id.max())} indexes the user table '
                             f'({self.user_num} rows) in get_items_reg')
        w = self._pair(train_teacher)[0]
        return 2. * InvPrefReg.apply(users_id, items_id, torch.zeros_like(users_id), norm, True, False, w, w,
                                     *self._stand_ins(self.user_num, self.user_num))

    def get_L1_reg(self, users_id, items_id, train_teacher):  # baseline_models.py:621-622 / :770-771
        return self._reg(users_id, items_id, 1, bool(train_teacher))

    def get_L2_reg(self, users_id, items_id, train_teacher):  # baseline_models.py:624-625 / :773-774
        return self._reg(users_id, items_id, 2, bool(train_teacher))

    # the pull of the student towards the detached teacher (baseline_models.py:634-649): plain tensor expressions -- the
    # managers never call them, their step forms the term inside csrc/invpref_cause.hip
    def item_teacher_reg(self, items_id):
        return torch.mean((self.item_emb(items_id) - self.teacher_item_emb(items_id).detach()) ** 2)

    def user_teacher_reg(self, users_id):
        return torch.mean((self.user_emb(users_id) - self.teacher_user_emb(users_id).detach()) ** 2)


class CausEMatrixFactorization(_CausEModelMixin, PureMatrixFactorization):
    """baseline_models.py:555-649.  A PureMatrixFactorization whose tables() lists the student pair first: predict(),
    recommend() and ImplicitTestManager's fused predict_topk route rank the student, as the reference's predict() does.
    get_L1_reg / get_L2_reg keep the reference's quirk: the item ids index the user table."""
    implicit = True


class CausEExplicitMatrixFactorization(_CausEModelMixin, PureExplicitMatrixFactorization):
    """baseline_models.py:706-794; predict(users, items) scores the student pair."""
    implicit = False


class _CausEManagerMixin(_OwnPassMixin, _UniformMixin):
    """CausETrainManager / CausEExplicitTrainManager (baseline_train.py:650-797):
        loss = train_score_loss + uniform_loss_coe * uniform_score_loss + L2_reg + teacher_reg_coe * teacher_reg
    with the student's score loss over the minibatch, the teacher's over the WHOLE uniform set at every step, L2_reg already
    weighted by L2_coe / teacher_L2_coe, and the student pulled towards the detached teacher ('i': item rows, 'u': user rows).
    Adam over all four tables; L1_coe is accepted and unused, like the reference's.

    The own-pass step of _OwnPassMixin on ops.cause_grad (csrc/invpref_cause.hip); the uniform set's inverted index is built
    once in the constructor."""
    _SINGLE = 'CausE runs in a single process (a sharded form would all-reduce the gradients of all four tables; not implemented)'
    _LOSS_KEYS = CAUSE_LOSS_KEYS
    _QUIRK = ('the reference\'s implicit CausE model indexes the user table ({U} rows) with item ids in get_items_reg and raises '
              'IndexError on {what} item id {i}; use item ids below user_num')

    def __init__(self, model, evaluator, device: torch.device, training_data: torch.Tensor, uniform_data: torch.Tensor,
                 batch_size: int, epochs: int, evaluate_interval: int, lr: float, L2_coe: float, L1_coe: float,
                 test_begin_epoch: int = 0, uniform_loss_coe: float = 1.0, teacher_reg_coe: float = 1.0,
                 teacher_reg_mode: str = 'i', teacher_L2_coe: float = 5., *, rank=None, world_size=None, process_group=None):
        if teacher_reg_mode not in ('i', 'u', 'ui'):
            raise ValueError(f'teacher_reg_mode must be \'i\', \'u\' or \'ui\', got {teacher_reg_mode!r}')
        self._require_single_process(world_size)
        if uniform_data is None or uniform_data.shape[0] == 0:
            raise ValueError('CausE needs a non-empty uniform set: its teacher trains on all of it at every step')
        if self.implicit:
            self._check_item_ids(model, training_data[:, 1], 'a training')
            self._check_item_ids(model, uniform_data[:, 1], 'a uniform')
        self._uniform_rows = int(uniform_data.shape[0])      # (the shared constructor sizes the workspace)
        super().__init__(model, evaluator, device, training_data, batch_size, epochs, evaluate_interval, lr, L2_coe, L1_coe,
                         test_begin_epoch, rank=rank, world_size=world_size, process_group=process_group)
        self.uniform_loss_coe, self.teacher_reg_coe = uniform_loss_coe, teacher_reg_coe
        self.teacher_reg_mode, self.teacher_L2_coe = teacher_reg_mode, teacher_L2_coe
        self._keep_uniform(uniform_data)
        self.uniform_user, self.uniform_item = self.uniform_user.contiguous(), self.uniform_item.contiguous()
        self.uniform_score = self.uniform_score.contiguous()
        self._uni_index = ops.macr_index_device(self.uniform_user, self.uniform_item, model.user_num, model.item_num, self.device)

    @classmethod
    def _check_item_ids(cls, model, items, what: str) -> None:
        if items.numel() and int(items.max()) >= model.user_num:
            raise ValueError(cls._QUIRK.format(U=model.user_num, what=what, i=int(items.max())))

    def _check_caller_batch(self, batch_users_tensor, batch_items_tensor) -> None:
        if self.implicit:
            self._check_item_ids(self.model, batch_items_tensor, 'a minibatch')

    def _workspace_bytes(self, batch: int) -> int:
        m = self.model
        return ops.cause_workspace_bytes(m.user_num, m.item_num, batch, self._uniform_rows, m.factor_num)

    def _own_pass(self, users, items, scores, index, losses6: torch.Tensor) -> None:
        st = self.state
        ops.cause_grad(st.p_views, st.g_views, users, items, scores, index, self.uniform_user, self.uniform_item,
                       self.uniform_score, self._uni_index, self.implicit, self.teacher_reg_mode, self.L2_coe,
                       self.teacher_L2_coe, self.uniform_loss_coe, self.teacher_reg_coe, losses6[:5], self._ws)


class CausETrainManager(_CausEManagerMixin, BasicImplicitTrainManager):
    """baseline_train.py:650-722 (baseline/general_bias_with_rct/CausE_mf_main.py)"""


class CausEExplicitTrainManager(_CausEManagerMixin, BasicExplicitTrainManager):
    """baseline_train.py:725-797 (baseline_explicit/general_bias_with_rct/CausE_mf_main.py)"""


# ------------------------------------------------------------------------------------------------ training on positives
def _kept_positives(training_data: torch.Tensor, weights, subject: str):
    """What a manager that trains on positives keeps of its constructor's data: -> (positives, keep, n_dropped, weights), the
    rows with a score > 0, their mask, the number of rows dropped and the fp32 weights (one per row of training_data, or per
    kept row) cut to the kept rows, or None"""
    keep = training_data[:, 2] > 0
    n_dropped = int(training_data.shape[0] - int(keep.sum()))
    if n_dropped == training_data.shape[0]:
        raise ValueError(f'{subject} trains on positives: training_data has no row with a score > 0')
    positives = training_data[keep]
    if weights is not None:
        w = torch.as_tensor(weights).detach().reshape(-1).to(torch.float32)
        if w.numel() == training_data.shape[0]:
            w = w[keep.to(w.device)]
        if w.numel() != positives.shape[0]:
            raise ValueError(f'weights holds {w.numel()} values for {training_data.shape[0]} rows / {len(positives)} positives')
        weights = w.contiguous()
    return positives, keep, n_dropped, weights


def _caller_positives(dev, batch_users_tensor, batch_items_tensor, batch_scores_tensor, subject: str):
    """The positives of a caller's minibatch, the rows with a score > 0: -> (users, items, B), int64 on `dev`"""
    keep = batch_scores_tensor.detach().reshape(-1).to(dev) > 0
    ud = batch_users_tensor.detach().to(dev).reshape(-1).to(torch.int64)[keep].contiguous()
    vd = batch_items_tensor.detach().to(dev).reshape(-1).to(torch.int64)[keep].contiguous()
    if ud.numel() == 0:
        raise ValueError(f'{subject} trains on positives: the minibatch has no row with a score > 0')
    return ud, vd, ud.numel()


# ------------------------------------------------------------------------------------------------ BPR-MF
class _TripletDrawnManager(_DeviceDrawnMixin, BasicImplicitTrainManager):
    """What the managers share that train on (user, positive item, negative item drawn on the device) triplets -- BPR-MF and
    LightGCN: BasicImplicitTrainManager's signature plus `seed`, `weights` and `exclude` (BPRTrainManager states them), the
    positives kept at construction, the exclusion lists, the draw launch (ops.bpr_draw), the staging rows (the step's users,
    then its negatives) and train_a_batch on caller tensors.  A manager supplies _SINGLE, _lazy_adam_unsupported,
    _workspace_bytes(), _own_pass() and, for what its pass needs beside the tables, _prepare_pass(positives), called once the
    engine stands and before the workspace is sized.  It may set _CALLER_SUBJECT, override _draw_caller() and _after_caller()
    (a caller's step: its draw; what follows however it ends) and set _TOUCHES where its model keeps final_tables(): the kernels
    write the parameters through raw pointers, so the model is told (touch()) behind every run of epochs and train_a_batch."""
    _CALLER_SUBJECT = 'BPR'     # who "trains on positives" in train_a_batch's error
    _TOUCHES = False

    def __init__(self, model, evaluator, device, training_data: torch.Tensor, batch_size: int, epochs: int,
                 evaluate_interval: int, lr: float, L2_coe: float, L1_coe: float, test_begin_epoch: int = 0, *, seed: int = 0,
                 weights=None, exclude=None, rank=None, world_size=None, process_group=None):
        self._require_single_process(world_size)
        positives, _, self.n_dropped, weights = _kept_positives(training_data, weights, 'BPR')
        super().__init__(model, evaluator, device, positives, batch_size, epochs, evaluate_interval, lr, L2_coe, L1_coe,
                         test_begin_epoch, rank=rank, world_size=world_size, process_group=process_group)
        U, I, dev = model.user_num, model.item_num, self.device
        if exclude is None:
            u, i = positives[:, 0].cpu().numpy().astype(np.int64), positives[:, 1].cpu().numpy().astype(np.int64)
            ok = (u >= 0) & (u < U) & (i >= 0) & (i < I)
            keys = np.unique(u[ok] * I + i[ok])      # (a pair that occurs twice is listed once; each user's items ascending)
            indptr = np.zeros(U + 1, np.int64)
            np.cumsum(np.bincount(keys // I, minlength=U), out=indptr[1:])
            exclude = (indptr, keys % I)
        self._excl = ops.device_csr(exclude, U, I, dev)
        self._weights = None if weights is None else weights.to(dev)
        self._prepare_pass(positives)
        self._init_device_draws(seed)

    def _prepare_pass(self, positives: torch.Tensor) -> None:
        """what the pass needs beside the tables, from the kept positives"""

    def _row_weights(self):
        return self._weights

    def _staging_resized(self, rows: int) -> None:
        super()._staging_resized(rows)
        self.n_forced = torch.zeros(rows, dtype=torch.int32, device=self.device)    # per step of the last staged run
        for k, b in enumerate(self._raw_batches):       # the minibatches are static: a row's users never change
            self._draws[k::self.batch_num, 0, :b.n] = b.users.to(torch.int32)

    def _draw_run(self, steps: int) -> None:
        ops.bpr_draw(self.users_tensor, self._step_lo[:steps], self._step_n[:steps], self._step_ids[:steps], self._excl,
                     self.model.item_num, self.seed, out=(self._draws[:steps, 1], self.n_forced[:steps]))

    def _enqueue_epochs(self, want: int) -> torch.Tensor:
        out = super()._enqueue_epochs(want)
        if self._TOUCHES:
            self.model.touch()
        return out

    def _draw_caller(self, ud: torch.Tensor, vd: torch.Tensor, B: int) -> torch.Tensor:
        """the negatives of a caller's step, int32 [1, B], drawn under the next step id"""
        return ops.bpr_draw(ud, torch.zeros(1, dtype=torch.int64, device=self.device), *self._step_name(B), self._excl,
                            self.model.item_num, self.seed, batch_cap=B)[0]

    def train_a_batch(self, batch_users_tensor, batch_items_tensor, batch_scores_tensor, *args) -> dict:
        """one step on caller tensors: the rows with a score > 0 are the positives (weight 1), their negatives are drawn under
        the next step id against the manager's exclusion lists (_draw_caller), this minibatch's index is built here"""
        dev, m = self.device, self.model
        try:
            ud, vd, B = _caller_positives(dev, batch_users_tensor, batch_items_tensor, batch_scores_tensor, self._CALLER_SUBJECT)
            neg = self._draw_caller(ud, vd, B)
            index = ops.bpr_index(ud, neg[0], m.item_num, m.user_num, vd)
            return self._caller_step(ud, vd, torch.ones(B, dtype=torch.float32, device=dev), neg, index, None)
        finally:
            self._after_caller()

    def _after_caller(self) -> None:
        """behind a caller's step, however it ended: what _draw_caller set aside is dropped, the model is told"""
        if self._TOUCHES:
            self.model.touch()


class BPRTrainManager(_TripletDrawnManager):
    """BPR-MF (Rendle et al., UAI 2009) on a plain PureMatrixFactorization: the pairwise ranking loss
        loss = mean_p w_p (-log sigmoid(Pu[u_p] . Qi[i_p] - Pu[u_p] . Qi[j_p])) + L2_coe * L2_reg + L1_coe * L1_reg
    over the training POSITIVES (u_p, i_p), each with a negative j_p drawn per step on the device, uniformly over the items
    outside the user's exclusion list (include/invpref_bpr.h states the loss and the draw rule).  BasicImplicitTrainManager's
    signature plus three keyword-only arguments:

    seed      names the trajectory: with the global step counter `step_id` it keys every draw, so the same seed gives the same
              bits whatever the run lengths, with graphs or without
    weights   one fp32 weight per positive (per row of training_data, or per kept row), e.g. the inverse propensities of
              ops.count_propensity: IPS-weighted BPR
    exclude   a CSR (indptr [user_num + 1], indices) of the items never drawn for a user; default: the user's training positives

    Rows of training_data with score <= 0 are dropped at construction (`n_dropped`); the static minibatches are taken over the
    positives in file order.  The device-drawn step of _DeviceDrawnMixin on ops.bpr_draw and ops.bpr_grad
    (csrc/invpref_bpr.hip); a staging row holds the step's users, then its negatives.  Single process."""
    _SINGLE = 'BPR runs in a single process (a sharded form would all-reduce the summed gradient of both tables; not implemented)'
    _lazy_adam_unsupported = ('the BPR pass stores zeros to every idle row and Adam runs over the whole tables: a lazy form '
                              'would update the rows the step\'s triplets touch (a follow-up)')

    def _workspace_bytes(self, batch: int) -> int:
        m = self.model
        return ops.bpr_workspace_bytes(m.user_num, m.item_num, batch, m.factor_num)

    def _own_pass(self, users, items, scores, draws, index, weights, losses6: torch.Tensor) -> None:
        st = self.state     # (draws[-1]: the negatives, of a staging row and of a caller's step, which stages them alone)
        ops.bpr_grad(st.p_views[0], st.p_views[1], users, items, draws[-1], index, self.L2_coe, self.L1_coe, st.g_views[0],
                     st.g_views[1], losses6[:4], weights=weights, workspace=self._ws)


# ------------------------------------------------------------------------------------------------ models ranked on derived tables
class _FinalTablesModel:
    """In front of nn.Module: a model scored on FINAL tables derived from its parameters (LightGCN's propagated tables, DICE's
    concatenation).  The model supplies final_tables() -> (F_user, F_item), detached, rebuilt when touch() was called since
    (the counter `_changes`, 0 from the model's constructor) or torch saw the parameters change.  The evaluators rank through
    rank_fn() / truth_rank_fn(): ops.predict_topk / ops.truth_ranks on final_tables(), no score matrix."""
    implicit = True

    def touch(self) -> None:
        """the parameters were written behind torch's back: the next final_tables() derives them again"""
        self._changes += 1

    def predict(self, users_id):
        """sigmoid(F_user[users] @ F_item^T) -> fp32 [n, item_num]"""
        F = self.final_tables()
        return ops.predict(F[0], F[1], _user_ids(users_id, F[0]), True)

    def rank_fn(self):
        """ImplicitTestManager's fused route: f(users, k, mask, highlight, truth) -> (items, scores, hits), ops.predict_topk on
        final_tables() as they are when rank_fn() is called"""
        F = self.final_tables()
        return lambda users, k, mask, highlight, truth: ops.predict_topk(F[0], F[1], users, k, True, mask=mask,
                                                                         highlight=highlight, truth=truth)

    def truth_rank_fn(self):
        """ImplicitRankTestManager's fused route: f(users, truth, mask, highlight) -> int32 ranks, ops.truth_ranks on
        final_tables()"""
        F = self.final_tables()
        return lambda users, truth, mask, highlight: ops.truth_ranks(F[0], F[1], users, truth, True, mask=mask,
                                                                     highlight=highlight)

    def recommend(self, users_id, k: int, exclude=None, highlight=None):
        """Each user's top-k items by the scores of predict() (InvPrefImplicit.recommend), on final_tables()"""
        F = self.final_tables()
        return ops.recommend(F[0], F[1], users_id, k, exclude, highlight)


# ------------------------------------------------------------------------------------------------ LightGCN
class LightGCNMatrixFactorization(_FinalTablesModel, nn.Module):
    """LightGCN (He et al., SIGIR 2020): the ego tables user_emb / item_emb (initialised as PureMF's) and the FINAL tables
        (F_user; F_item) = (1 / (K + 1)) sum_{k = 0 .. K} A^k (user_emb; item_emb),   K = n_layers,
    A the symmetrically normalised user-item graph handed in by set_graph() (ops.lgcn_graph; csrc/invpref_lgcn.hip).  A pair is
    scored by sigmoid(F_user[u] . F_item[i]).

    Not a PureMatrixFactorization: the evaluators must not take the ego tables for ranking tables (_FinalTablesModel's routes).

    final_tables() keeps its result and recomputes it when set_graph() or touch() was called since, or when the ego parameters
    were replaced or written in place through torch (their data pointers and torch version counters are compared).  The
    kernels of this package write the tables through raw pointers, which torch's counters do not see: LightGCNTrainManager
    calls touch() behind every run of epochs and every train_a_batch; whoever else writes the tables that way calls it too.
    The result is written into the same two buffers every time, so a pair returned earlier follows the model."""

    def __init__(self, user_num: int, item_num: int, factor_num: int, n_layers: int = 3):
        super().__init__()
        if not 0 <= int(n_layers) <= _capi.LGCN_MAX_LAYERS:
            raise ValueError(f'n_layers must lie in 0 .. {_capi.LGCN_MAX_LAYERS}')
        self.user_num, self.item_num, self.factor_num, self.n_layers = user_num, item_num, factor_num, int(n_layers)
        self.user_emb = nn.Embedding(user_num, factor_num)
        self.item_emb = nn.Embedding(item_num, factor_num)
        nn.init.normal_(self.user_emb.weight, std=0.01)
        nn.init.normal_(self.item_emb.weight, std=0.01)
        self.graph = None
        self._changes, self._final, self._final_key, self._ws = 0, None, None, None

    def tables(self):
        """the EGO pair, the flat state of a manager (not what ranks: final_tables())"""
        return [self.user_emb.weight, self.item_emb.weight]

    def set_graph(self, graph) -> None:
        if (graph.user_num, graph.item_num) != (self.user_num, self.item_num):
            raise ValueError(f'a graph of {graph.user_num} x {graph.item_num} for tables of {self.user_num} x {self.item_num}')
        self.graph = graph
        self.touch()

    def final_tables(self):
        """(F_user, F_item), detached; see the class docstring for when they are recomputed"""
        if self.graph is None:
            raise RuntimeError('LightGCNMatrixFactorization: set_graph(ops.lgcn_graph(...)) first')
        P, Q = self.user_emb.weight, self.item_emb.weight
        key = (self._changes, P.data_ptr(), Q.data_ptr(), P._version, Q._version)
        if key != self._final_key:
            if self.graph.device != P.device:
                self.graph = self.graph.to(P.device)
            if self._final is None or self._final[0].device != P.device:
                self._final = (torch.empty_like(P.detach()), torch.empty_like(Q.detach()))
                self._ws = ops.Workspace(P.device)
            ops.lgcn_propagate(self.graph, P.detach().contiguous(), Q.detach().contiguous(), self.n_layers, out=self._final,
                               workspace=self._ws)
            self._final_key = key
        return self._final


class LightGCNTrainManager(_TripletDrawnManager):
    """LightGCN trained with BPR: BPRTrainManager's loss with the scores taken on the model's FINAL tables and the regulariser
    on its EGO tables,
        loss = mean_p w_p (-log sigmoid(F_u[u_p] . F_i[i_p] - F_u[u_p] . F_i[j_p])) + L2_coe * L2_reg + L1_coe * L1_reg,
    BPRTrainManager's signature (seed, weights, exclude), draws, staging rows and run index.  The graph is built from the kept
    positives at construction (ops.lgcn_graph: the distinct in-range pairs) and handed to the model.  One step is four enqueued
    calls, all capturable: ops.lgcn_propagate (ego -> F), ops.bpr_grad on F without a regulariser (-> GF), ops.lgcn_propagate
    (GF -> the ego gradient: the operator is its own adjoint), ops.lgcn_reg into the same gradient and losses; then the
    engine's dense / ranged Adam.  F, GF and the workspace are sized once at construction.  Single process."""
    _SINGLE = ('LightGCN runs in a single process (a sharded form would exchange every layer\'s tables between the ranks; '
               'not implemented)')
    _lazy_adam_unsupported = ('lazy Adam updates the rows a minibatch names, but the propagation reaches every row: the '
                              'gradient of the ego tables is dense')
    _TOUCHES = True

    def _prepare_pass(self, positives: torch.Tensor) -> None:
        m, dev = self.model, self.device
        u, i = positives[:, 0].cpu().to(torch.int64), positives[:, 1].cpu().to(torch.int64)
        ok = (u >= 0) & (u < m.user_num) & (i >= 0) & (i < m.item_num)
        self.graph = ops.lgcn_graph(u[ok], i[ok], m.user_num, m.item_num, device=dev)
        m.set_graph(self.graph)
        shape = lambda rows: torch.zeros(rows, m.factor_num, dtype=torch.float32, device=dev)   # noqa: E731
        self._F = (shape(m.user_num), shape(m.item_num))       # the final tables of the step
        self._GF = (shape(m.user_num), shape(m.item_num))      # the gradient of the final tables

    def _workspace_bytes(self, batch: int) -> int:
        m = self.model     # (the four calls of a step follow each other on one stream and carry nothing in the workspace)
        sizes = (ops.bpr_workspace_bytes(m.user_num, m.item_num, batch, m.factor_num),
                 ops.lgcn_workspace_bytes(self.graph, m.factor_num), ops.lgcn_reg_workspace_bytes(m.user_num, m.item_num))
        return 0 if 0 in sizes else max(sizes)

    def _own_pass(self, users, items, scores, draws, index, weights, losses6: torch.Tensor) -> None:
        st, K, F, GF = self.state, self.model.n_layers, self._F, self._GF
        ops.lgcn_propagate(self.graph, st.p_views[0], st.p_views[1], K, out=F, workspace=self._ws)
        ops.bpr_grad(F[0], F[1], users, items, draws[-1], index, 0.0, 0.0, GF[0], GF[1], losses6[:4], weights=weights,
                     workspace=self._ws)
        ops.lgcn_propagate(self.graph, GF[0], GF[1], K, out=(st.g_views[0], st.g_views[1]), workspace=self._ws)
        ops.lgcn_reg(users, items, draws[-1], st.p_views[0], st.p_views[1], self.L2_coe, self.L1_coe, st.g_views[0],
                     st.g_views[1], losses6[:4], workspace=self._ws)


# ------------------------------------------------------------------------------------------------ DICE
DICE_LOSS_KEYS = ('click_loss', 'int_loss', 'con_loss', 'dis', 'L2_reg', 'loss')
_DICE_LOSS_PICK = (0, 1, 2, 3, 4, 6)        # their places in the pass's losses8 (include/invpref_dice.h)


class DICEMatrixFactorization(_FinalTablesModel, nn.Module):
    """DICE (Zheng et al., WWW 2021): an interest pair int_user_emb / int_item_emb and a conformity pair con_user_emb /
    con_item_emb, all four initialised as PureMF's.  A pair is scored by sigmoid(F_user[u] . F_item[i]) on the FINAL tables,

    rank_by='interest'   the interest pair alone: the paper's choice under intervened test data
    rank_by='both'       [Iu | Cu] and [Ii | Ci], width 2 factor_num: the click score, interest + conformity; the ranking
                         kernels take rows of at most INVPREF_MAX_FACTORS floats, so factor_num <= 128

    Not a PureMatrixFactorization: _FinalTablesModel's routes rank it.  For 'both', final_tables() keeps the concatenation
    and rebuilds it when touch() was called since, or when the parameters were replaced or written in place through torch
    (their data pointers and torch version counters are compared), as LightGCNMatrixFactorization does: DICETrainManager calls
    touch() behind every run of epochs and every train_a_batch, since the kernels write the tables through raw pointers.  The
    concatenation is written into the same two buffers every time, so a pair returned earlier follows the model."""

    def __init__(self, user_num: int, item_num: int, factor_num: int, rank_by: str = 'both'):
        super().__init__()
        if rank_by not in ('interest', 'both'):
            raise ValueError(f"rank_by must be 'interest' or 'both', got {rank_by!r}")
        if rank_by == 'both' and 2 * int(factor_num) > _capi.DEFINES['MAX_FACTORS']:
            raise ValueError(f"rank_by='both' ranks rows of 2 factor_num = {2 * int(factor_num)} floats and the ranking kernels "
                             f"take at most {_capi.DEFINES['MAX_FACTORS']}: factor_num <= {_capi.DEFINES['MAX_FACTORS'] // 2}, "
                             "or rank_by='interest'")
        self.user_num, self.item_num, self.factor_num, self.rank_by = user_num, item_num, factor_num, rank_by
        self.int_user_emb = nn.Embedding(user_num, factor_num)
        self.int_item_emb = nn.Embedding(item_num, factor_num)
        self.con_user_emb = nn.Embedding(user_num, factor_num)
        self.con_item_emb = nn.Embedding(item_num, factor_num)
        for e in (self.int_user_emb, self.int_item_emb, self.con_user_emb, self.con_item_emb):
            nn.init.normal_(e.weight, std=0.01)
        self._changes, self._final, self._final_key = 0, None, None

    def tables(self):
        """Iu, Ii, Cu, Ci: the flat state of a manager (not what ranks: final_tables())"""
        return [self.int_user_emb.weight, self.int_item_emb.weight, self.con_user_emb.weight, self.con_item_emb.weight]

    def final_tables(self):
        """(F_user, F_item), detached; see the class docstring"""
        T = self.tables()
        if self.rank_by == 'interest':
            return T[0].detach(), T[1].detach()
        key = (self._changes,) + tuple(x for t in T for x in (t.data_ptr(), t._version))
        if key != self._final_key:
            D = self.factor_num
            if self._final is None or self._final[0].device != T[0].device:
                self._final = tuple(torch.empty(t.shape[0], 2 * D, dtype=torch.float32, device=t.device) for t in T[:2])
            for F, a, b in zip(self._final, T[:2], T[2:]):
                F[:, :D].copy_(a.detach())
                F[:, D:].copy_(b.detach())
            self._final_key = key
        return self._final


def dice_schedule(epoch: int, margin: float, int_weight: float, con_weight: float, dis_pen: float, margin_decay: float,
                  loss_decay: float):
    """(margin, (int_w, con_w, dis_pen)) of epoch `epoch`, counted from 0: margin and the two loss weights decay per epoch"""
    return margin * margin_decay ** epoch, (int_weight * loss_decay ** epoch, con_weight * loss_decay ** epoch, dis_pen)


class DICETrainManager(_TripletDrawnManager):
    """DICE on a DICEMatrixFactorization: per step, over the training POSITIVES (u_p, i_p), each with a negative j_p drawn on
    the device CONDITIONED ON THE POSITIVE'S POPULARITY (the popularity-margin sampler),
        loss = click_loss + int_w * int_loss + con_w * con_loss - dis_pen * dis + L2_coe * L2_reg + L1_coe * L1_reg
    with the click loss on interest + conformity, the interest loss on the triplets whose negative is the more popular item,
    the conformity loss following popularity and the discrepancy between the two pairs over the step's distinct rows
    (include/invpref_dice.h states the terms, the factors and the draw rule).  BPRTrainManager's signature (seed, weights,
    exclude) plus keyword-only arguments:

    margin, pool     the sampler's popularity margin and the least size of a candidate range
    int_weight, con_weight, dis_pen   the three coefficients
    dis_form         'L1' or 'L2': the discrepancy's phi
    margin_decay, loss_decay   epoch e, counted from the manager's first, uses margin * margin_decay ** e, int_weight *
                     loss_decay ** e and con_weight * loss_decay ** e

    The per-epoch values of a run's steps are written to device rows (`_step_margin`, `_step_coefs`) before the run is enqueued,
    next to the step ids; the draw launch and the passes read their rows when they run, so a captured run is replayed at
    the current values without re-capture.  A caller's step (train_a_batch) runs at the current epoch's.  The popularity
    arrays are built from the kept positives (ops.dice_popularity).  The device-drawn step of _DeviceDrawnMixin on
    ops.dice_draw and ops.dice_grad (csrc/invpref_dice.hip); a staging row holds the step's users, then its negatives.  Single
    process."""
    _SINGLE = ('DICE runs in a single process (a sharded form would all-reduce the summed gradient of all four tables and the '
               'counts of distinct rows; not implemented)')
    _LOSS_KEYS = DICE_LOSS_KEYS
    _lazy_adam_unsupported = ('the DICE pass stores zeros to every idle row and Adam runs over the whole tables: a lazy form '
                              'would update the rows the step\'s triplets touch (not built)')
    _CALLER_SUBJECT = 'DICE'
    _TOUCHES = True

    def __init__(self, model, evaluator, device, training_data: torch.Tensor, batch_size: int, epochs: int,
                 evaluate_interval: int, lr: float, L2_coe: float, L1_coe: float, test_begin_epoch: int = 0, *, seed: int = 0,
                 weights=None, exclude=None, margin: float = 40.0, pool: int = 40, int_weight: float = 0.1,
                 con_weight: float = 0.1, dis_pen: float = 0.01, dis_form: str = 'L1', margin_decay: float = 0.9,
                 loss_decay: float = 0.9, rank=None, world_size=None, process_group=None):
        self._require_single_process(world_size)
        if not callable(getattr(model, 'tables', None)) or len(model.tables()) != 4:
            raise TypeError('DICETrainManager needs a model with an interest and a conformity pair (DICEMatrixFactorization)')
        if dis_form not in ops.DICE_FORMS:
            raise ValueError(f'dis_form must be one of {sorted(ops.DICE_FORMS)}, got {dis_form!r}')
        if int(pool) < 1:
            raise ValueError(f'pool must be at least 1, got {pool}')
        for name, v in (('margin', margin), ('int_weight', int_weight), ('con_weight', con_weight), ('dis_pen', dis_pen),
                        ('margin_decay', margin_decay), ('loss_decay', loss_decay)):
            if not (np.isfinite(float(v)) and float(v) >= 0.0):
                raise ValueError(f'{name} must be a finite number >= 0, got {v}')
        self.margin, self.pool, self.dis_form = float(margin), int(pool), dis_form
        self.int_weight, self.con_weight, self.dis_pen = float(int_weight), float(con_weight), float(dis_pen)
        self.margin_decay, self.loss_decay = float(margin_decay), float(loss_decay)
        self._row = self._caller_coefs = None
        super().__init__(model, evaluator, device, training_data, batch_size, epochs, evaluate_interval, lr, L2_coe, L1_coe,
                         test_begin_epoch, seed=seed, weights=weights, exclude=exclude, rank=rank, world_size=world_size,
                         process_group=process_group)

    def schedule_of(self, epoch: int):
        """(margin, (int_w, con_w, dis_pen)) of epoch `epoch`, counted from the manager's first"""
        return dice_schedule(epoch, self.margin, self.int_weight, self.con_weight, self.dis_pen, self.margin_decay,
                             self.loss_decay)

    def _prepare_pass(self, positives: torch.Tensor) -> None:
        self._pop = ops.dice_popularity(positives[:, 1], self.model.item_num, self.device)
        self._losses8 = torch.zeros(8, dtype=torch.float32, device=self.device)
        self._loss_pick = torch.tensor(_DICE_LOSS_PICK, dtype=torch.int64, device=self.device)

    def _workspace_bytes(self, batch: int) -> int:
        m = self.model
        return ops.dice_workspace_bytes(m.user_num, m.item_num, batch, m.factor_num)

    def _staging_resized(self, rows: int) -> None:
        super()._staging_resized(rows)
        self._step_margin = torch.zeros(rows, dtype=torch.float64, device=self.device)
        self._step_coefs = torch.zeros(rows, 3, dtype=torch.float64, device=self.device)

    def _draw_run(self, steps: int) -> None:
        # the run's epochs start at epoch_cnt: their margins and coefficients into the steps' rows, then the draw launch
        sched = [self.schedule_of(self.epoch_cnt + e) for e in range(steps // self.batch_num)]
        self._step_margin[:steps].copy_(torch.from_numpy(np.repeat([m for m, _ in sched], self.batch_num)))
        self._step_coefs[:steps].copy_(torch.from_numpy(np.repeat(np.array([c for _, c in sched], np.float64), self.batch_num, 0)))
        ops.dice_draw(self.users_tensor, self.items_tensor, self._step_lo[:steps], self._step_n[:steps], self._step_ids[:steps],
                      self._excl, self._pop, self.pool, self._step_margin[:steps], self.seed,
                      out=(self._draws[:steps, 1], self.n_forced[:steps]))

    def _gradient_pass(self, k, plan, users, items, envs, scores, weights, batch_norm: int, coefs, flags: int,
                       losses6: torch.Tensor, sched=None) -> None:
        self._row = None if k is None else self._loss_slot * self.batch_num + k     # the step's row of _step_coefs
        super()._gradient_pass(k, plan, users, items, envs, scores, weights, batch_norm, coefs, flags, losses6, sched)

    def _own_pass(self, users, items, scores, draws, index, weights, losses6: torch.Tensor) -> None:
        st = self.state
        coefs3 = self._caller_coefs if self._row is None else self._step_coefs[self._row]
        ops.dice_grad(st.p_views, st.g_views, users, items, draws[-1], self._pop[0], index, coefs3, self.dis_form, self.L2_coe,
                      self.L1_coe, self._losses8, weights=weights, workspace=self._ws)
        torch.index_select(self._losses8, 0, self._loss_pick, out=losses6)

    def _draw_caller(self, ud: torch.Tensor, vd: torch.Tensor, B: int) -> torch.Tensor:
        """at the current epoch's margin; its coefficients are set aside for the pass (_own_pass: a step without a row)"""
        dev = self.device
        margin, coefs3 = self.schedule_of(self.epoch_cnt)
        self._caller_coefs = torch.tensor(coefs3, dtype=torch.float64, device=dev)
        return ops.dice_draw(ud, vd, torch.zeros(1, dtype=torch.int64, device=dev), *self._step_name(B), self._excl, self._pop,
                             self.pool, torch.full((1,), margin, dtype=torch.float64, device=dev), self.seed, batch_cap=B)[0]

    def _after_caller(self) -> None:
        self._caller_coefs = None
        super()._after_caller()


# ------------------------------------------------------------------------------------------------ sampled-softmax MF
class SSMTrainManager(_StagedRunMixin, _WholePassMixin, BasicImplicitTrainManager):
    """Sampled-softmax MF on a plain PureMatrixFactorization: the softmax loss over a positive and M sampled negatives
        loss = mean_p w_p (logsumexp(x_p+, x_p0 .. x_pM-1) - x_p+) + L2_coe * L2_reg + L1_coe * L1_reg
        x_p+ = Pu[u_p] . Qi[i_p] / temperature      x_pk = Pu[u_p] . Qi[n_k] / temperature + item_bias[n_k]
    over the training POSITIVES (u_p, i_p); the M negatives n_k are drawn per step on the device and SHARED by all positions of
    the step (include/invpref_ssm.h states the loss, the accidental-hit mask and the draw rule).  BasicImplicitTrainManager's
    signature plus keyword-only arguments:

    n_neg        M, the negatives of a step
    temperature  tau > 0
    beta         the negatives are drawn with probability q proportional to (training count + 1) ** beta; 0: uniformly
    correct      add the sampling correction -log(n_neg q) to the negatives' logits (the importance-sampling estimate of the
                 full-catalogue softmax); False: plain sampled softmax, which penalises what the proposal draws often
    proposal     an explicit (cum, item_bias) in the form of ops.ssm_proposal (either may be None) instead of beta / correct
    seed         names the trajectory: with the global step counter `step_id` it keys every draw, so the same seed gives the
                 same bits whatever the run lengths, with graphs or without
    weights      one fp32 weight per positive (per row of training_data, or per kept row)

    Rows of training_data with score <= 0 are dropped at construction (`n_dropped`); the static minibatches are taken over the
    positives in file order, and each one's inverted index (ops.ssm_index) is built once.  A staging row of _StagedRunMixin is
    the step's M negatives: before a run of epochs is enqueued its steps are named step_id + 0, 1, ... and ONE ops.ssm_draw
    launch fills their rows; the pass (ops.ssm_grad, csrc/invpref_ssm.hip) reads its row when it runs, so whole epochs
    replay as graphs with new negatives.  A caller's minibatch (train_a_batch) is one step under the next step id.  Single
    process."""
    _SINGLE = ('sampled-softmax MF runs in a single process (a sharded form would all-reduce the summed gradient of both '
               'tables; not implemented)')
    _lazy_adam_unsupported = ('the sampled-softmax pass stores zeros to every idle row and Adam runs over the whole tables: a '
                              'lazy form would update the rows the step\'s positives and negatives touch (a follow-up)')

    def __init__(self, model, evaluator, device, training_data: torch.Tensor, batch_size: int, epochs: int,
                 evaluate_interval: int, lr: float, L2_coe: float, L1_coe: float, test_begin_epoch: int = 0, *, n_neg: int = 256,
                 temperature: float = 1.0, beta: float = 0.0, correct: bool = True, proposal=None, seed: int = 0, weights=None,
                 rank=None, world_size=None, process_group=None):
        self._require_single_process(world_size)
        if not 1 <= int(n_neg) <= _capi.SSM_MAX_NEG:
            raise ValueError(f'n_neg must lie in [1, {_capi.SSM_MAX_NEG}], got {n_neg}')
        if not (float(temperature) > 0.0 and np.isfinite(float(temperature))):
            raise ValueError(f'temperature must be a positive finite number, got {temperature}')
        positives, _, self.n_dropped, weights = _kept_positives(training_data, weights, 'sampled softmax')
        super().__init__(model, evaluator, device, positives, batch_size, epochs, evaluate_interval, lr, L2_coe, L1_coe,
                         test_begin_epoch, rank=rank, world_size=world_size, process_group=process_group)
        I, dev = model.item_num, self.device
        self.n_neg, self.temperature, self.beta, self.correct = int(n_neg), float(temperature), float(beta), bool(correct)
        if proposal is None:
            i = positives[:, 1].cpu().numpy().astype(np.int64)
            counts = np.bincount(i[(i >= 0) & (i < I)], minlength=I)
            proposal = ops.ssm_proposal(counts, self.beta, self.n_neg, self.correct)
        cum, bias = proposal
        self._cum = None if cum is None else torch.as_tensor(cum).detach().reshape(-1).to(torch.int32).contiguous().to(dev)
        self._bias = None if bias is None else torch.as_tensor(bias).detach().reshape(-1).to(torch.float32).contiguous().to(dev)
        for t, what in ((self._cum, 'cum'), (self._bias, 'item_bias')):
            if t is not None and t.numel() != I:
                raise ValueError(f'proposal: {what} holds {t.numel()} entries for {I} items')
        self._weights = None if weights is None else weights.to(dev)
        self.seed, self.step_id = int(seed), 0
        self._caller = None         # train_a_batch: (users, items, negatives, index) of the caller's minibatch
        self._pos_index = None      # per static minibatch: ops.ssm_index of its positives
        self._ws = ops.Workspace(dev)
        self._ws.get(max(self._workspace_bytes(min(batch_size, self.n_total)), 16))   # sized once: capturable launches
        self._init_staging(self.n_neg)

    def _workspace_bytes(self, batch: int) -> int:
        m = self.model
        return ops.ssm_workspace_bytes(m.user_num, m.item_num, batch, self.n_neg, m.factor_num)

    def _staging_resized(self, rows: int) -> None:
        self._step_ramp = torch.arange(rows, dtype=torch.int64, device=self.device)
        self._step_ids = torch.zeros(rows, dtype=torch.int64, device=self.device)

    def _raw_setup(self):
        super()._raw_setup()
        if self._pos_index is None:
            m = self.model
            self._pos_index = [ops.ssm_index(b.users, b.items, m.user_num, m.item_num) for b in self._raw_batches]

    def _stage_draws(self, n: int) -> None:
        steps = n * self.batch_num
        torch.add(self._step_ramp[:steps], self.step_id, out=self._step_ids[:steps])
        ops.ssm_draw(self._step_ids[:steps], self.model.item_num, cum=self._cum, seed=self.seed, out=self._staged[:steps])

    def _draws_consumed(self, steps: int) -> None:
        self.step_id += steps

    def _gradient_pass(self, k, plan, users, items, envs, scores, weights, batch_norm: int, coefs, flags: int,
                       losses6: torch.Tensor, sched=None) -> None:
        if k is None:
            users, items, neg, index = self._caller
            w = None
        else:
            b, w = self._raw_batches[k], self._weights
            neg, index = self._staged[self._loss_slot * self.batch_num + k], self._pos_index[k]
            w = None if w is None else w[b.lo:b.lo + b.n]
        st = self.state
        ops.ssm_grad(st.p_views[0], st.p_views[1], users, items, neg, index, self.temperature, self.L2_coe, self.L1_coe,
                     st.g_views[0], st.g_views[1], losses6[:4], weights=w, item_bias=self._bias, workspace=self._ws)

    def train_a_batch(self, batch_users_tensor, batch_items_tensor, batch_scores_tensor, *args) -> dict:
        """one step on caller tensors: the rows with a score > 0 are the positives (weight 1), the negatives are drawn under
        the next step id, this minibatch's index is built here"""
        dev, m = self.device, self.model
        ud, vd, B = _caller_positives(dev, batch_users_tensor, batch_items_tensor, batch_scores_tensor, 'sampled softmax')
        neg = ops.ssm_draw(torch.full((1,), self.step_id, dtype=torch.int64, device=dev), m.item_num, self.n_neg, cum=self._cum,
                           seed=self.seed)[0]
        self._ws.get(max(self._workspace_bytes(B), 16))
        self._caller = (ud, vd, neg, ops.ssm_index(ud, vd, m.user_num, m.item_num))
        try:
            out = self._batch_step(ud, vd, torch.ones(B, dtype=torch.float32, device=dev), None, lambda: None)
        finally:
            self._caller = None
        self.step_id += 1
        return out


# ------------------------------------------------------------------------------------------------ doubly robust MF
DR_LOSS_KEYS = ('score_loss', 'imputation_loss', 'L2_reg', 'L1_reg', 'loss')


class _DRModelMixin:
    """What DRMatrixFactorization and its explicit twin add to a PureMF model: the imputation pair imp_user_emb / imp_item_emb,
    an MF of the same shape that predicts the prediction model's error (include/invpref_dr.h), initialised N(0, 0.01) after
    the prediction pair (state_dict order: user_emb, item_emb, imp_user_emb, imp_item_emb)."""

    def __init__(self, user_num: int, item_num: int, factor_num: int):
        super().__init__(user_num, item_num, factor_num)
        self.imp_user_emb = nn.Embedding(user_num, factor_num)
        self.imp_item_emb = nn.Embedding(item_num, factor_num)
        nn.init.normal_(self.imp_user_emb.weight, std=0.01)
        nn.init.normal_(self.imp_item_emb.weight, std=0.01)

    def tables(self):
        """the four tables in state_dict order: the prediction pair first, so whatever ranks tables()[0] . tables()[1] ranks
        the prediction model"""
        return [self.user_emb.weight, self.item_emb.weight, self.imp_user_emb.weight, self.imp_item_emb.weight]

    def imputation(self, users_id, items_id):
        """the imputation model at the pairs: the soft pseudo-label sigmoid(z) (implicit) or the imputed score z (explicit),
        z = imp_user_emb[u] . imp_item_emb[i]; a plain tensor expression"""
        z = (self.imp_user_emb(users_id) * self.imp_item_emb(items_id)).sum(-1)
        return torch.sigmoid(z) if self.implicit else z


class DRMatrixFactorization(_DRModelMixin, PureMatrixFactorization):
    """A PureMatrixFactorization with an imputation pair: predict(), recommend() and the Implicit*TestManagers' fused routes rank
    the prediction pair."""
    implicit = True


class DRExplicitMatrixFactorization(_DRModelMixin, PureExplicitMatrixFactorization):
    """A PureExplicitMatrixFactorization with an imputation pair; predict(users, items) scores the prediction pair."""
    implicit = False


class _DRManagerMixin(_DeviceDrawnMixin):
    """Doubly robust joint learning (Wang et al., ICML 2019) on a DR*MatrixFactorization: per step, over the B rows of a
    minibatch with inverse propensities w and as many pairs drawn uniformly from the whole user x item grid,
        loss = score_loss + imputation_loss + L2_coe * L2_reg + L1_coe * L1_reg
        score_loss      = [sum_observed w d + sum_drawn e^] / B        imputation_loss = [sum_observed w d^2] / B
    with e^ the error the imputation model predicts and d = e - e^ (include/invpref_dr.h states both forms, the factors and
    the draw rule).  JOINT learning with SIMULTANEOUS updates: both gradients are taken at the same parameters, the cross terms
    detached (score_loss sees the imputation tables as constants and imputation_loss the prediction tables, as CausE's step
    detaches its teacher), and ONE Adam step moves all four tables.  It is not the paper's alternating two-optimiser loop; it
    keeps the engine's one-Adam-per-step sequence and its device-side schedule as they are.

    Basic*TrainManager's signature plus keyword-only arguments:

    seed             names the trajectory: with the global step counter `step_id` it keys every draw, so the same seed gives
                     the same bits whatever the run lengths, with graphs or without
    weights          one fp32 inverse propensity per row of training_data
    propensity_func  basic_item_ / basic_user_ / basic_pair_propensity_func: the weights are formed on the device from the
                     interaction counts (smooth_weight_coe their exponent), as the IPS managers form theirs, and kept as
                     inverse_propensity_tensor.  Neither given: every weight is 1.  Both given: ValueError.

    The device-drawn step of _DeviceDrawnMixin on ops.dr_draw and ops.dr_grad (csrc/invpref_dr.hip; every row of the four
    gradients overwritten); a staging row holds the step's drawn users, then its drawn items.  Single process."""
    _SINGLE = ('doubly robust MF runs in a single process (a sharded form would all-reduce the summed gradient of all four '
               'tables; not implemented)')
    _LOSS_KEYS = DR_LOSS_KEYS
    _lazy_adam_unsupported = ('the doubly robust pass stores zeros to every idle row, its drawn pairs reach rows outside the '
                              'minibatch and Adam runs over the whole tables: a lazy form is not built')

    def __init__(self, model, evaluator, device, training_data: torch.Tensor, batch_size: int, epochs: int,
                 evaluate_interval: int, lr: float, L2_coe: float, L1_coe: float, test_begin_epoch: int = 0, *, seed: int = 0,
                 weights=None, propensity_func=None, smooth_weight_coe: float = 1.0, rank=None, world_size=None,
                 process_group=None):
        self._require_single_process(world_size)
        if weights is not None and propensity_func is not None:
            raise ValueError('give weights or propensity_func, not both')
        if propensity_func is not None and propensity_func not in _COUNT_KINDS:
            raise ValueError('propensity_func must be basic_item_propensity_func, basic_user_propensity_func or '
                             'basic_pair_propensity_func')
        if len(model.tables()) != 4:
            raise TypeError(f'{type(self).__name__} needs a model with an imputation pair (DRMatrixFactorization / '
                            'DRExplicitMatrixFactorization)')
        if weights is not None:
            weights = torch.as_tensor(weights).detach().reshape(-1).to(torch.float32)
            if weights.numel() != training_data.shape[0]:
                raise ValueError(f'weights holds {weights.numel()} values for {training_data.shape[0]} rows')
        super().__init__(model, evaluator, device, training_data, batch_size, epochs, evaluate_interval, lr, L2_coe, L1_coe,
                         test_begin_epoch, rank=rank, world_size=world_size, process_group=process_group)
        self.smooth_weight_coe, self.propensity_func = smooth_weight_coe, propensity_func
        U, I, dev = model.user_num, model.item_num, self.device
        self.inverse_propensity_tensor = None
        if weights is not None:
            self.inverse_propensity_tensor = weights.contiguous().to(dev)
        elif propensity_func is not None:
            cnt = ops.interaction_counts(self.users_tensor, self.items_tensor, U, I)
            self.inverse_propensity_tensor = ops.count_propensity(*cnt, self.users_tensor, self.items_tensor,
                                                                  _COUNT_KINDS[propensity_func], smooth_weight_coe)
        self._init_device_draws(seed)

    def _workspace_bytes(self, batch: int) -> int:
        m = self.model
        return ops.dr_workspace_bytes(m.user_num, m.item_num, batch, m.factor_num)

    def _row_weights(self):
        return self.inverse_propensity_tensor

    def _draw_run(self, steps: int) -> None:
        m = self.model
        ops.dr_draw(self._step_n[:steps], self._step_ids[:steps], m.user_num, m.item_num, self.seed, out=self._draws[:steps])

    def _own_pass(self, users, items, scores, draws, index, weights, losses6: torch.Tensor) -> None:
        st = self.state
        ops.dr_grad(0 if self.implicit else 1, st.p_views, st.g_views, users, items, scores, draws[0], draws[1], index,
                    self.L2_coe, self.L1_coe, losses6[:5], weights=weights, workspace=self._ws)

    def train_a_batch(self, batch_users_tensor, batch_items_tensor, batch_scores_tensor, weight_tensor=None) -> dict:
        """one step on caller tensors (weight_tensor: the rows' inverse propensities, None: 1): as many pairs as the minibatch
        has rows are drawn under the next step id, this minibatch's index is built here"""
        dev, m = self.device, self.model
        ud = batch_users_tensor.detach().to(dev).reshape(-1).to(torch.int64).contiguous()
        vd = batch_items_tensor.detach().to(dev).reshape(-1).to(torch.int64).contiguous()
        B = ud.numel()
        if B == 0:
            raise ValueError('an empty minibatch')
        w = None if weight_tensor is None else weight_tensor.detach().to(dev).float().reshape(-1).contiguous()
        if w is not None and w.numel() != B:
            raise ValueError(f'weight_tensor holds {w.numel()} values for {B} rows')
        draws = ops.dr_draw(*self._step_name(B), m.user_num, m.item_num, self.seed, batch_cap=B)[0]
        index = ops.dr_index(ud, vd, draws[0], draws[1], m.user_num, m.item_num)
        return self._caller_step(ud, vd, batch_scores_tensor, draws, index, w)


class DRTrainManager(_DRManagerMixin, BasicImplicitTrainManager):
    """doubly robust MF on implicit feedback (form 0: BCE against the soft pseudo-label) over a DRMatrixFactorization"""


class DRExplicitTrainManager(_DRManagerMixin, BasicExplicitTrainManager):
    """doubly robust MF on explicit feedback (form 1: squared error) over a DRExplicitMatrixFactorization"""


# ------------------------------------------------------------------------------------------------ list-based managers
# ALS, EASE and Mult-DAE are not epoch-engine managers (no row plans, no minibatches of interactions): each sits directly on the
# engine's outer loop and shares what follows.
def _interactions(training_data):
    """training_data -> CPU (users int64, items int64, label as stored), rows of (user, item, label)"""
    data = torch.as_tensor(training_data).detach().cpu()
    if data.dim() != 2 or data.shape[1] < 3 or data.shape[0] < 1:
        raise ValueError('training_data holds rows of (user, item, label)')
    return data[:, 0].to(torch.int64), data[:, 1].to(torch.int64), data[:, 2]


def _require_finite_tables(model) -> None:
    for t in model.tables():
        if not bool(torch.isfinite(t.detach()).all()):
            raise ValueError('the model\'s tables hold non-finite values')


class _ErrorWordMixin:
    """The device's sticky error word of a manager whose kernels report a failed pivot there (and count, in n_skipped, the
    entries they left out): both zeroed at construction, never cleared; check_error() reads the word and raises."""
    _ERROR = None                   # the manager's message, around {word}

    def _init_error_word(self, device) -> None:
        self.n_skipped = torch.zeros(1, dtype=torch.int32, device=device)
        self.error_word = torch.zeros(1, dtype=torch.int32, device=device)

    def check_error(self) -> None:
        word = int(self.error_word.item())
        if word:
            raise _capi.InvPrefError(self._ERROR.format(word=word))


ALS_LOSS_KEYS = ['fit_loss', 'L2_reg', 'loss']


class ALSTrainManager(_ErrorWordMixin, _OuterLoop):
    """Weighted matrix factorization solved as Hu, Koren and Volinsky (ICDM 2008) solve it: alternating least squares on a
    plain PureMatrixFactorization (include/invpref_als.h states the model).  Row e of training_data is the entry (user, item,
    label): preference p_e = 1 if label > 0 else 0 (a listed 0 is an observed negative), confidence c_e = 1 + alpha * w_e with w_e the label or the caller's `weights` (one value per
    row, >= 0); every other user x item pair carries confidence 1 and preference 0, and a row listed twice counts twice.  One
    sweep solves every user row exactly against the item table, then every item row against the new user table
    (ops.als_gram / ops.als_solve: float64 normal equations and Cholesky, one rounding to fp32), then evaluates
        loss = fit_loss + reg * L2_reg      L2_reg = |X|^2 + |Y|^2
    with ops.als_objective.  No learning rate, no negative sampling, no minibatches: not an epoch-engine manager (no row plans,
    no Adam), only the engine's outer loop; an "epoch" is a sweep.  Single process.

    The tables are the model's own parameters, written in place.  Negative weights, non-finite tables and ids outside the
    tables are refused at construction, on the host; the device's sticky error word (a failed pivot: a NaN that reached a
    table) is checked at every read-back and raises InvPrefError.

    Fold-in: `fold_in(item_lists)` solves users that were not in training against the trained item table, e.g.
        rows = mgr.fold_in([[3, 17, 4], [8]])                                     # fp32 [2, D]
        items, scores = ops.recommend(rows, model.item_emb.weight, torch.arange(2, device=rows.device), k=10)
    """

    _LOSS_KEYS = ALS_LOSS_KEYS
    _ERROR = ('ALS: a row\'s normal matrix was not positive definite or its solution not finite (error word {word}): a NaN '
              'reached a table, or a confidence was below 1; the affected rows are NaN')

    def __init__(self, model, evaluator, device: torch.device, training_data: torch.Tensor, epochs: int, evaluate_interval: int,
                 reg: float, alpha: float, *, weights=None, test_begin_epoch: int = 0):
        if not isinstance(model, PureMatrixFactorization):
            raise TypeError('ALSTrainManager takes a PureMatrixFactorization')
        if model.factor_num > _capi.ALS_MAX_FACTORS:
            raise _capi.InvPrefError(f'factor_num {model.factor_num}: the ALS solve takes at most {_capi.ALS_MAX_FACTORS} factors')
        if not reg > 0:
            raise ValueError('reg must be > 0: it is what keeps every normal matrix positive definite')
        users, items, label = _interactions(training_data)
        label = label.to(torch.float32)
        w = label if weights is None else torch.as_tensor(weights).detach().cpu().reshape(-1).to(torch.float32)
        if w.numel() != label.numel():
            raise ValueError(f'weights holds {w.numel()} values for {label.numel()} rows')
        if not bool(torch.isfinite(w).all()) or bool((w < 0).any()):
            raise ValueError('weights (the labels by default) must be finite and >= 0: a confidence below 1 can lose positive '
                             'definiteness')
        _require_finite_tables(model)
        self.model, self.evaluator, self.device = model.to(device), evaluator, torch.device(device)
        self.epochs, self.evaluate_interval, self.test_begin_epoch = int(epochs), int(evaluate_interval), int(test_begin_epoch)
        self.reg, self.alpha = float(reg), float(alpha)
        self.epoch_cnt, self.n_total = 0, int(label.numel())
        dev = self.device
        conf = 1.0 + self.alpha * w
        pref = (label > 0).to(torch.float32)
        self.by_user, self.by_item = ops.als_csr(users.to(dev), items.to(dev), pref.to(dev), conf.to(dev), model.user_num,
                                                 model.item_num)
        D = model.factor_num
        self._gram = torch.zeros(D, D, dtype=torch.float64, device=dev)
        self._init_error_word(dev)
        self._ws = ops.Workspace(dev)
        if dev.type == 'cuda':      # sized once: every later launch is capturable
            U, I, n = model.user_num, model.item_num, self.n_total
            self._ws.get(max(ops.als_workspace_bytes(U, I, n, D), ops.als_workspace_bytes(I, U, n, D), 16))

    def _tables(self):
        return self.model.user_emb.weight.detach(), self.model.item_emb.weight.detach()

    # ---- the launches; nothing here reads back
    def train_user_half(self) -> None:
        """every user row against the item table as it is"""
        X, Y = self._tables()
        ops.als_gram(Y, self.reg, out=self._gram, workspace=self._ws)
        ops.als_solve(Y, self._gram, self.by_user, X, n_skipped=self.n_skipped, error_word=self.error_word, workspace=self._ws)

    def train_item_half(self) -> None:
        X, Y = self._tables()
        ops.als_gram(X, self.reg, out=self._gram, workspace=self._ws)
        ops.als_solve(X, self._gram, self.by_item, Y, n_skipped=self.n_skipped, error_word=self.error_word, workspace=self._ws)

    def objective_into(self, out3: torch.Tensor) -> torch.Tensor:
        """float64 (fit_loss, L2_reg, loss) of the tables as they are, into out3 on the device"""
        X, Y = self._tables()
        ops.als_gram(Y, self.reg, out=self._gram, workspace=self._ws)
        return ops.als_objective(X, Y, self._gram, self.reg, self.by_user, out=out3, workspace=self._ws)

    def enqueue_sweep(self, out3: torch.Tensor) -> None:
        """one sweep -- user half, item half, objective -- enqueued on the current stream (capturable)"""
        self.train_user_half()
        self.train_item_half()
        self.objective_into(out3)

    # ---- read-backs
    def read_back(self, dev_losses: torch.Tensor) -> list:
        """the loss dicts of a [n, 3] device tensor, after the check of the sticky error word"""
        self.check_error()
        return self.loss_dicts(dev_losses)

    def objective(self) -> dict:
        out = self.objective_into(torch.empty(3, dtype=torch.float64, device=self.device))
        return self.read_back(out)[0]

    def train_a_sweep(self) -> dict:
        return self.train_epochs(1)[0]

    train_a_epoch = train_a_sweep

    def train_epochs(self, n: int, sync: bool = True):
        """n sweeps enqueued back to back.  sync: ONE read-back -> the n loss dicts; otherwise the float64 [n, 3] device tensor
        (read it with read_back)."""
        losses = torch.empty(max(int(n), 0), 3, dtype=torch.float64, device=self.device)
        for k in range(int(n)):
            self.enqueue_sweep(losses[k])
            self.epoch_cnt += 1
        return self.read_back(losses) if sync else losses

    # ---- fold-in
    def fold_in(self, item_lists, pref=None, conf=None) -> torch.Tensor:
        """The vectors of users given by their item lists, solved against the item table as it is and its Gram matrix: the user
        half-sweep on a batch of arbitrary lists (the row_ids form of the same kernel) -> fp32 [n, D].  pref / conf: per list, one
        value per item; default preference 1 and confidence 1 + alpha.  A user without items gets zeros."""
        n, total = len(item_lists), sum(len(l) for l in item_lists)
        D, dev = self.model.factor_num, self.device
        if n < 1 or total < 1:
            return torch.zeros(n, D, dtype=torch.float32, device=dev)

        def flat(values, default):
            if values is None:
                return torch.full((total,), default, dtype=torch.float32)
            v = torch.cat([torch.as_tensor(x, dtype=torch.float32).reshape(-1) for x in values])
            if v.numel() != total:
                raise ValueError('fold_in: pref / conf hold one value per listed item')
            return v
        row_ptr, cols = ops.lists_csr(item_lists, self.model.item_num, dev, 'fold_in')
        p, c = flat(pref, 1.0), flat(conf, 1.0 + self.alpha)
        if bool((c < 1).any()) or not bool(torch.isfinite(c).all() and torch.isfinite(p).all()):
            raise ValueError('fold_in: confidences must be finite and >= 1, preferences finite')
        csr = (row_ptr, cols, c.to(dev), p.to(dev))
        _, Y = self._tables()
        gram = ops.als_gram(Y, self.reg)
        out = torch.empty(n, D, dtype=torch.float32, device=dev)
        ops.als_solve(Y, gram, csr, out, row_ids=torch.arange(n, dtype=torch.int32, device=dev), n_skipped=self.n_skipped,
                      error_word=self.error_word)
        self.check_error()
        return out


class _HistoryModel:
    """What the models that score a user from the list of its training items share (EASE, Mult-DAE), in front of nn.Module: the
    training lists by user as buffers (`hist_ptr` int64 [user_num + 1], `hist_cols` int32), so that the model scores its
    training users from its state_dict alone; arbitrary lists as a CSR (fold-in); recommend() in bounded batches over the
    model's predict()."""

    def _init_history(self) -> None:
        self.register_buffer('hist_ptr', torch.zeros(self.user_num + 1, dtype=torch.int64))
        self.register_buffer('hist_cols', torch.zeros(0, dtype=torch.int32))

    def set_history(self, by_user) -> None:
        """the training lists by user, as ops.ease_lists gives them"""
        row_ptr, cols = by_user
        if row_ptr.numel() != self.user_num + 1:
            raise ValueError(f'the lists name {row_ptr.numel() - 1} users, the model has {self.user_num}')
        dev = self.hist_ptr.device
        self.hist_ptr = row_ptr.to(dev, torch.int64).contiguous()
        self.hist_cols = cols.to(dev, torch.int32).contiguous()

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        cols = state_dict.get(prefix + 'hist_cols')
        if cols is not None and cols.shape != self.hist_cols.shape:   # (the one buffer whose length is the data's)
            self.hist_cols = torch.zeros(cols.shape, dtype=torch.int32, device=self.hist_cols.device)
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def _lists_csr(self, item_lists):
        """(row_ptr int64 [n + 1], cols int32) on the model's device of users given by their item lists"""
        return ops.lists_csr(item_lists, self.item_num, self.hist_ptr.device, 'predict_lists')

    def _history_of(self, users):
        """(ptr int32 [n + 1], items int32) of the training lists of `users`, gathered on the device"""
        start = self.hist_ptr[users]
        lens = self.hist_ptr[users + 1] - start
        ptr = torch.zeros(users.numel() + 1, dtype=torch.int64, device=users.device)
        ptr[1:] = torch.cumsum(lens, 0)
        at = torch.arange(int(ptr[-1]), device=users.device) + torch.repeat_interleave(start - ptr[:-1], lens)
        items = self.hist_cols[at] if at.numel() else torch.zeros(1, dtype=torch.int32, device=users.device)
        return ptr.to(torch.int32), items.contiguous()

    def recommend(self, users_id, k: int, exclude=True):
        """Each user's top-k items by predict()'s scores -> (items int32 [n, k], scores fp32 [n, k]).  exclude: True leaves out
        the user's training items.  Score matrices of at most 1 GiB at a time, as the evaluators bound theirs."""
        users = users_id.reshape(-1).to(torch.int64)
        n, k = users.numel(), int(k)
        step = max(1, min(n, (1 << 28) // max(1, self.item_num + (3 * k if k > _capi.MAX_TOPK else 0))))
        items, scores = [], []
        for lo in range(0, n, step):
            batch = users[lo:lo + step]
            got = ops.topk_rows(self.predict(batch), k, mask=self._history_of(batch) if exclude else None)
            items.append(got[0])
            scores.append(got[1])
        if not items:
            dev = self.hist_ptr.device
            return torch.empty(0, k, dtype=torch.int32, device=dev), torch.empty(0, k, dtype=torch.float32, device=dev)
        return (items[0], scores[0]) if len(items) == 1 else (torch.cat(items), torch.cat(scores))


class EASEModel(_HistoryModel, nn.Module):
    """EASE (Steck, WWW 2019): the item-item ridge model, score(u, .) = x_u . B with x_u the user's training counts and B fp32
    [item_num, item_num] of zero diagonal (include/invpref_ease.h states the model).  `weight` is B, a parameter without
    gradient: zeros until EASETrainManager.fit() has written it.  The training lists by user are buffers (`hist_ptr` int64
    [user_num + 1], `hist_cols` int32), so that the model scores its training users from its state_dict alone.  Ranking is by
    the raw score, no sigmoid: the evaluators take the model through predict()."""

    def __init__(self, user_num: int, item_num: int):
        super().__init__()
        if not 1 <= int(item_num) <= _capi.EASE_MAX_ITEMS or int(user_num) < 1:
            raise _capi.InvPrefError(f'EASEModel: {user_num} users x {item_num} items; EASE takes 1 .. {_capi.EASE_MAX_ITEMS} items')
        self.user_num, self.item_num = int(user_num), int(item_num)
        self.weight = nn.Parameter(torch.zeros(self.item_num, self.item_num), requires_grad=False)
        self._init_history()

    def predict(self, users_id) -> torch.Tensor:
        """fp32 [n, item_num]: the raw scores of the training users `users_id` (an id outside the table scores zero)"""
        users = users_id.reshape(-1).to(torch.int32)
        return ops.ease_scores(self.weight.detach(), (self.hist_ptr, self.hist_cols), list_ids=users)

    def predict_lists(self, item_lists) -> torch.Tensor:
        """Fold-in: fp32 [n, item_num], the scores of users given by their item lists (an item listed twice counts twice) -- the
        same kernel on arbitrary lists, nothing refitted."""
        if len(item_lists) < 1:
            return torch.zeros(0, self.item_num, dtype=torch.float32, device=self.weight.device)
        return ops.ease_scores(self.weight.detach(), self._lists_csr(item_lists))


class EASETrainManager(_ErrorWordMixin, _OuterLoop):
    """Fits an EASEModel in closed form: row e of training_data is (user, item, label), and x_ui counts the rows of (u, i) with
    label > 0 (a pair listed twice counts twice).  fit() is three launches -- ops.ease_gram (X^T X + reg I, exact integers),
    ops.spd_inverse (float64, blocked, in place) and ops.ease_weights (one rounding to fp32 into the model's weight) -- with one
    hyper-parameter, no learning rate and no sampling: not an epoch-engine manager, only the engine's outer loop, whose one
    "epoch" is the fit.  Single process.

    reg <= 0, ids outside the tables, non-finite labels and counts beyond the Gram kernel's counters are refused at
    construction, on the host; the device's sticky error word (a pivot that was not positive) is read after the fit and raises
    InvPrefError.  keep_inverse keeps the float64 inverse of X^T X + reg I in `inverse` (8 item_num^2 bytes)."""

    _ERROR = ('EASE: X^T X + reg I was not positive definite in float64 or its inverse not finite (error word {word}); the '
              'weights are NaN')
    epochs, evaluate_interval, test_begin_epoch = 1, 1, 0       # the outer loop's: evaluate, fit, evaluate

    def __init__(self, model, evaluator, device: torch.device, training_data: torch.Tensor, reg: float, *,
                 keep_inverse: bool = False):
        if not isinstance(model, EASEModel):
            raise TypeError('EASETrainManager takes an EASEModel')
        reg = float(reg)
        if not (reg > 0 and reg < float('inf')):
            raise ValueError('reg must be finite and > 0: it is what keeps X^T X + reg I positive definite')
        users, items, label = _interactions(training_data)
        if not bool(torch.isfinite(torch.as_tensor(training_data).to(torch.float64)).all()):
            raise ValueError('training_data holds non-finite values')
        self.model, self.evaluator, self.device = model.to(device), evaluator, torch.device(device)
        self.reg, self.keep_inverse = reg, bool(keep_inverse)
        self.epoch_cnt, self.n_total = 0, int(label.numel())
        dev = self.device
        self.lists = ops.ease_lists(users.to(dev), items.to(dev), label.to(dev), model.user_num, model.item_num)
        self.model.set_history(self.lists[0])
        self._init_error_word(dev)
        self.inverse = None

    def enqueue_fit(self) -> None:
        """the three launches on the current stream; nothing is read back"""
        _, _, _, self.inverse = ops.ease_fit(self.lists, self.reg, out=self.model.weight.detach(), keep_inverse=self.keep_inverse,
                                             n_skipped=self.n_skipped, error_word=self.error_word)
        self.epoch_cnt = 1

    def fit(self) -> None:
        self.enqueue_fit()
        self.check_error()

    # ---- train(): the engine's outer loop around the fit -- the evaluation at "epoch" 0 (the zero weights), the fit, the
    # evaluation at epoch 1 -> ([{}], [1]), (tests, [0, 1]).  The closed form has no loss to report: the one loss dict is empty.
    def train_epochs(self, n: int = 1, sync: bool = True):
        """the fit, enqueued; the error word is read at the end of train()"""
        self.enqueue_fit()
        losses = torch.empty(1, 0, device=self.device)
        return self.read_back(losses) if sync else losses

    def read_back(self, dev_losses: torch.Tensor) -> list:
        return [{} for _ in range(dev_losses.shape[0])]

    def _after_training(self) -> None:
        self.check_error()


# ------------------------------------------------------------------------------------------------ Mult-DAE
MULTDAE_LOSS_KEYS = ['score_loss', 'L2_reg', 'loss']


class MultDAEModel(_HistoryModel, nn.Module):
    """Mult-DAE (Liang, Krishnan, Hoffman and Jebara, WWW 2018) with the paper's architecture [I -> D -> I]: z_u = tanh(enc_bias +
    s_u sum of the rows of `enc` the user's list names), scores z_u . dec[j] + dec_bias[j] over the whole catalogue
    (include/invpref_multdae.h states the model).  No user table: a user is the list of its items, so predict_lists() scores
    users that were not in training.  The training lists by user are buffers (`hist_ptr`, `hist_cols`), as EASEModel's.  Xavier-
    normal tables and zero biases from torch's generator.  Ranking is by the raw logit: the evaluators take the model through
    predict()."""

    def __init__(self, user_num: int, item_num: int, factor_num: int):
        super().__init__()
        if int(user_num) < 1 or int(item_num) < 1 or not 1 <= int(factor_num) <= _capi.DEFINES['MAX_FACTORS']:
            raise _capi.InvPrefError(f'MultDAEModel: {user_num} users x {item_num} items, factor_num {factor_num}; the kernels '
                                     f'take 1 .. {_capi.DEFINES["MAX_FACTORS"]} factors')
        self.user_num, self.item_num, self.factor_num = int(user_num), int(item_num), int(factor_num)
        self.enc = nn.Parameter(nn.init.xavier_normal_(torch.empty(self.item_num, self.factor_num)), requires_grad=False)
        self.enc_bias = nn.Parameter(torch.zeros(self.factor_num), requires_grad=False)
        self.dec = nn.Parameter(nn.init.xavier_normal_(torch.empty(self.item_num, self.factor_num)), requires_grad=False)
        self.dec_bias = nn.Parameter(torch.zeros(self.item_num), requires_grad=False)
        self._init_history()

    def tables(self):
        return [self.enc, self.enc_bias, self.dec, self.dec_bias]

    def _scores(self, lists, list_ids: torch.Tensor) -> torch.Tensor:
        """the encoder at p = 0, the score product, the bias"""
        z = ops.multdae_encode(self.enc.detach(), self.enc_bias.detach(), lists, list_ids)
        scores = ops.predict(z, self.dec.detach(), torch.arange(z.shape[0], device=z.device), sigmoid=False)
        return scores.add_(self.dec_bias.detach())

    def predict(self, users_id) -> torch.Tensor:
        """fp32 [n, item_num]: the raw logits of the training users `users_id` (an id outside the table scores as an empty
        list)"""
        return self._scores((self.hist_ptr, self.hist_cols), users_id.reshape(-1).to(torch.int32))

    def predict_lists(self, item_lists) -> torch.Tensor:
        """Fold-in: fp32 [n, item_num], the logits of users given by their item lists (an item listed twice counts twice) -- the
        same kernels on arbitrary lists, nothing refitted."""
        n = len(item_lists)
        if n < 1:
            return torch.zeros(0, self.item_num, dtype=torch.float32, device=self.enc.device)
        return self._scores(self._lists_csr(item_lists), torch.arange(n, dtype=torch.int32, device=self.enc.device))


class MultDAETrainManager(_OuterLoop, _SingleProcessMixin):
    """Trains a MultDAEModel by gradient steps on the multinomial likelihood over the WHOLE catalogue (ops.multdae_grad: no [B, I]
    array) with Adam.  Row e of training_data is (user, item, label); rows with label <= 0 are dropped, a pair listed twice
    counts twice (the lists come from ops.ease_lists, so at most INVPREF_EASE_MAX_ITEMS items and its count limit: refused
    here by name).  Not an epoch-engine manager, only the engine's outer loop: its minibatches are USERS, batch_size
    consecutive ones, static, each one's inverted index built once.  One flat buffer holds the four parameters (the model's
    parameters are views of it), likewise the gradients and Adam's two moments: a step is the pass plus ONE ops.adam_ launch.
    The dropout mask of a step is named by (seed, the global step counter): the same seed gives the same bits whatever the run
    lengths.  Single process."""
    _LOSS_KEYS = MULTDAE_LOSS_KEYS
    _SINGLE = 'Mult-DAE trains in a single process: its step sweeps the whole catalogue per user and shares no row plan to shard'

    def __init__(self, model, evaluator, device: torch.device, training_data: torch.Tensor, batch_size: int, epochs: int,
                 evaluate_interval: int, lr: float, L2_coe: float, *, dropout: float = 0.5, seed: int = 0,
                 test_begin_epoch: int = 0, world_size=None):
        self._require_single_process(world_size)
        if not isinstance(model, MultDAEModel):
            raise TypeError('MultDAETrainManager takes a MultDAEModel')
        if model.item_num > _capi.EASE_MAX_ITEMS:   # (ops.ease_lists, which builds the training lists, stops there)
            raise _capi.InvPrefError(f'MultDAETrainManager: {model.item_num} items; the training lists come from ops.ease_lists, '
                                     f'which takes at most {_capi.EASE_MAX_ITEMS} (the pass itself takes any catalogue: '
                                     f'ops.multdae_grad on lists of the caller\'s)')
        if not 0.0 <= float(dropout) < 1.0:
            raise ValueError('dropout must lie in [0, 1)')
        if int(batch_size) < 1 or int(batch_size) > _capi.MULTDAE_MAX_BATCH:
            raise ValueError(f'batch_size must lie in 1 .. {_capi.MULTDAE_MAX_BATCH} users')
        if not (float(lr) > 0 and float(L2_coe) >= 0):
            raise ValueError('lr must be > 0 and L2_coe >= 0')
        users, items, label = _interactions(training_data)
        _require_finite_tables(model)
        self.model, self.evaluator, self.device = model.to(device), evaluator, torch.device(device)
        self.batch_size, self.epochs, self.evaluate_interval = int(batch_size), int(epochs), int(evaluate_interval)
        self.test_begin_epoch, self.lr, self.L2_coe = int(test_begin_epoch), float(lr), float(L2_coe)
        self.dropout, self.seed = float(dropout), int(seed)
        self.epoch_cnt, self.step_cnt = 0, 0
        dev = self.device
        by_user, _ = ops.ease_lists(users.to(dev), items.to(dev), label.to(dev), model.user_num, model.item_num)
        self.lists = by_user
        self.model.set_history(by_user)
        # one flat buffer, each tensor from a multiple of four floats: the tables' rows stay 16-byte aligned
        shapes = [tuple(t.shape) for t in model.tables()]
        sizes = [int(np.prod(s)) for s in shapes]
        offsets = np.cumsum([0] + [(n + 3) // 4 * 4 for n in sizes])
        self._flat = torch.zeros(int(offsets[-1]), dtype=torch.float32, device=dev)
        self._grad, self._exp_avg, self._exp_avg_sq = (torch.zeros_like(self._flat) for _ in range(3))
        self._params, self._grads = [], []
        for t, o, n, s in zip(model.tables(), offsets, sizes, shapes):
            view = self._flat[int(o):int(o) + n].view(s)
            view.copy_(t.detach())
            t.data = view
            self._params.append(view)
            self._grads.append(self._grad[int(o):int(o) + n].view(s))
        self.batches = []
        for lo in range(0, model.user_num, self.batch_size):
            users = torch.arange(lo, min(lo + self.batch_size, model.user_num), dtype=torch.int32, device=dev)
            self.batches.append((users, ops.multdae_index(self.lists, users, model.item_num)))
        self._ws = ops.Workspace(dev)
        self._ws.get(max(self._workspace_bytes(users, index) for users, index in self.batches))

    def _workspace_bytes(self, users, index) -> int:
        n2 = (index.numel() - users.numel() - 1) // 5
        return ops.multdae_workspace_bytes(self.model.item_num, users.numel(), n2, self.model.factor_num)

    def _step(self, users, index, step_word: torch.Tensor, losses3: torch.Tensor) -> None:
        """the pass and ONE Adam launch over the flat buffers"""
        ops.multdae_grad(self._params, self._grads, self.lists, users, index, self.dropout, self.seed, step_word, self.L2_coe,
                         losses3, workspace=self._ws)
        self.step_cnt += 1
        ops.adam_(self._flat, self._grad, self._exp_avg, self._exp_avg_sq, self.step_cnt, self.lr)

    def train_epochs(self, n: int, sync: bool = True):
        """n epochs over the static minibatches, enqueued back to back; the steps' ids are one arange on the device.  sync: ONE
        read-back -> the n loss dicts; otherwise the fp32 [n, 3] device tensor (read it with read_back)."""
        n, nb = max(int(n), 0), len(self.batches)
        step_ids = torch.arange(self.step_cnt, self.step_cnt + n * nb, dtype=torch.int64, device=self.device)
        losses = torch.empty(n, nb, 3, dtype=torch.float32, device=self.device)
        for k in range(n):
            for b, (users, index) in enumerate(self.batches):
                self._step(users, index, step_ids[k * nb + b:k * nb + b + 1], losses[k, b])
            self.epoch_cnt += 1
        out = losses.mean(1) if n else losses.reshape(0, 3)
        return self.read_back(out) if sync else out

    def train_a_epoch(self) -> dict:
        return self.train_epochs(1)[0]

    @staticmethod
    def caller_users(users, user_num: int) -> torch.Tensor:
        """a caller's list of users as int32 list ids, checked on the host: 1 .. INVPREF_MULTDAE_MAX_BATCH ids inside the lists"""
        users = torch.as_tensor(users).detach().cpu().reshape(-1)
        if users.numel() < 1 or users.numel() > _capi.MULTDAE_MAX_BATCH:
            raise ValueError(f'train_a_batch takes 1 .. {_capi.MULTDAE_MAX_BATCH} users')
        if users.dtype.is_floating_point or users.dtype == torch.bool:
            raise ValueError('train_a_batch takes integer user ids')
        if int(users.min()) < 0 or int(users.max()) >= int(user_num):
            raise ValueError('train_a_batch: a user id lies outside the training lists')
        return users.to(torch.int32)

    def train_a_batch(self, users) -> dict:
        """one step on a caller's list of users (list ids of the training lists); its index is built here"""
        users = self.caller_users(users, self.model.user_num).to(self.device)
        index = ops.multdae_index(self.lists, users, self.model.item_num)
        self._ws.get(self._workspace_bytes(users, index))
        losses = torch.empty(3, dtype=torch.float32, device=self.device)
        self._step(users, index, torch.tensor([self.step_cnt], dtype=torch.int64, device=self.device), losses)
        return self.loss_dicts(losses)[0]
