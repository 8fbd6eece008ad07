"""Drop-in ``ImplicitTrainManager`` / ``ExplicitTrainManager`` (reference train.py:16-342, :693-1019).

Same constructor signature, public attributes, method names and return shapes as the reference;
the work inside is re-designed for MI355X:

* the seven parameter tensors are re-homed as views of ONE flat fp32 buffer (with flat gradient
  and Adam-moment twins), so the optimiser is a single fused HIP launch and multi-GPU needs a
  single RCCL all-reduce per step;
* ``train_a_batch`` = fused M-step HIP kernel (forward + 3 losses + 2 regularisers + analytic
  backward + scatter-add) -> [all-reduce] -> fused zero_grad+Adam kernel;
* ``cluster`` + ``stat_envs`` = one E-step launch over all local interactions + one finish launch;
* no per-batch host syncs: ``train_a_epoch`` reads the loss terms back once per epoch.

Sharding (parallel.py): with ``world_size`` G > 1 every rank keeps only its share of
every minibatch ``[kB,(k+1)B)`` -- by default (round 6: what BASELINE.json's north_star names) a contiguous row
slice, parameters replicated, ONE all-reduce of the flat gradient per optimiser step (INVPREF_EXCHANGE=scatter |
packed: the same sums as reduce-scatter + all-gather / over the touched rows only); with INVPREF_SHARD=users the
interactions of the users it owns (only the item-side gradient is all-reduced).
Every mean() keeps the GLOBAL batch length as denominator, so summing the per-rank gradient
buffers reproduces the single-GPU gradient.

The epoch loop, the flat state, the step sequences, the graphs and the exchanges are the epoch engine's (engine.py); this
module holds what is InvPref's own and answers the engine's hooks with it.
"""
from __future__ import annotations

import math
import os
from typing import Optional

import numpy as np
import torch

from . import _capi, ops
from . import plan as planlib
from .engine import (LOSS_KEYS, FlatState, RawBatch, _EpochEngine, _gc_paused, touched_row_offsets,  # noqa: F401 (re-exported)
                     transfer_loss_dict_to_line_str)
from .parallel import all_reduce_sum_


class _InvPrefTrainManager(_EpochEngine):
    """The epoch engine (engine.py) + what is InvPref's own: the environments and the E-step, the lazily kept sample weights
    and class weights, the alpha schedule and the cluster events of the outer loop."""
    implicit = True
    _pure = False                       # the step's kernel form: all seven tables
    _make_tables = staticmethod(_capi.make_tables)

    def __init__(
            self, model, evaluator, device: torch.device, training_data: torch.Tensor, batch_size: int,
            epochs: int, cluster_interval: int, evaluate_interval: int, lr: float,
            invariant_coe: float, env_aware_coe: float, env_coe: float, L2_coe: float, L1_coe: float,
            alpha: float = None, use_class_re_weight: bool = False, test_begin_epoch: int = 0,
            begin_cluster_epoch: int = None, stop_cluster_epoch: int = None, cluster_use_random_sort: bool = True,
            use_recommend_re_weight: bool = True, *, rank: Optional[int] = None, world_size: Optional[int] = None,
            process_group=None,
    ):
        self.envs_num: int = model.env_num
        self._env_count = self.envs_num     # (the row plans lay a minibatch out per environment)
        self._init_engine(model, evaluator, device, training_data, batch_size, epochs, evaluate_interval, lr, L2_coe, L1_coe,
                          test_begin_epoch, rank, world_size, process_group,
                          flags=ops.flags_of(self.implicit, use_recommend_re_weight, use_class_re_weight,
                                             model.reg_only_embed, model.reg_env_embed),
                          # user-sharded: [Pu | Pa | Qi | Qa | Ev | W | b]: the replicated part (items + small tables) and the
                          # loss tail form one contiguous range for the all-reduce, the owned user rows two ranges for Adam
                          users_first=[0, 2, 1, 3, 4, 5, 6], env_switches=True)
        # initial environments: one numpy draw over ALL rows, like the reference (train.py:34),
        # then this rank keeps its rows -> identical to the single-GPU run for any world size
        envs_all = torch.from_numpy(np.random.randint(0, self.envs_num, self.n_total).astype(np.int64))
        self.envs = (envs_all.index_select(0, self.shard.local_rows()) if self.world_size > 1 else envs_all).to(self.device)

        self.cluster_interval = cluster_interval
        self.invariant_coe, self.env_aware_coe, self.env_coe = invariant_coe, env_aware_coe, env_coe
        self.each_env_count = dict()
        if alpha is None:
            self.alpha, self.update_alpha = 0., True
        else:
            self.alpha, self.update_alpha = alpha, False
        self.use_class_re_weight = use_class_re_weight
        self.use_recommend_re_weight = use_recommend_re_weight
        # sample_weights[i] = class_weights[envs[i]] (train.py:274-278).  The N-length array is kept LAZILY on one GPU: stat_envs()
        # refreshes class_weights and the planned M-step kernels look the weight up by environment (INVPREF_WEIGHTS_BY_ENV);
        # the array is materialised when somebody reads the `sample_weights` attribute (property below).
        self._sample_weights = torch.zeros(self.users_tensor.shape[0], dtype=torch.float32, device=self.device)
        self._sw_lazy = False        # True: _sample_weights is behind (it equals class_weights[envs] once materialised)
        self._by_env = False         # True: class_weights[envs] IS what the reference's sample_weights would hold right now
        self._epoch_by_env = False   # what the epochs being issued / captured use (fixed per _enqueue_epochs call)
        self._counts_dev = torch.zeros(self.envs_num, dtype=torch.int64, device=self.device)
        self._es = None              # ops.EstepState of the fused E-step (one GPU)
        self._estep_graphs = {}
        self.class_weights = torch.zeros(self.envs_num, dtype=torch.float32, device=self.device)
        self.begin_cluster_epoch, self.stop_cluster_epoch = begin_cluster_epoch, stop_cluster_epoch
        self.cluster_use_random_sort = cluster_use_random_sort
        self._eps_base = np.array([1e-10 * (1e-1 ** i) for i in range(self.envs_num)], dtype=np.float32)
        self._eps_rows_cnt = math.factorial(self.envs_num)

    # ------------------------------------------------------------------ sample weights (train.py:67, :274-278)
    @property
    def sample_weights(self) -> torch.Tensor:
        """The reference's attribute.  Read from outside, the array is brought up to date first; and because the caller may
        write into it (the reference's loop only slices it), the epochs fall back to reading it per interaction until the next
        stat_envs() re-establishes sample_weights == class_weights[envs]."""
        self._materialise_sample_weights()
        self._by_env = False
        return self._sample_weights

    @sample_weights.setter
    def sample_weights(self, value: torch.Tensor):
        self._sample_weights, self._sw_lazy, self._by_env = value, False, False

    def _materialise_sample_weights(self):
        if self._sw_lazy:
            _, sw = ops.sample_weights(self.envs, self._counts_dev, self.n_total, self.envs_num)   # class_weights[envs]
            self._sample_weights.copy_(sw)
            self._sw_lazy = False

    def _step_weights(self, bw):
        """(weights argument, flags) of one of the epochs' planned launches: the minibatch's slice of the sample-weight array, or
        -- INVPREF_WEIGHTS_BY_ENV -- the E class weights the kernel indexes by environment"""
        if bw is not None and self._epoch_by_env:
            return self.class_weights, self._flags | _capi.WEIGHTS_BY_ENV
        return bw, self._flags

    def _weights_by_env(self) -> bool:
        """may the epochs' launches take an interaction's weight as class_weights[env]? (one GPU, planned M-step, weights
        consistent with the environments: stat_envs() ran since they last changed, nobody was handed the array since);
        INVPREF_WEIGHTS_BY_ENV=0 (test hook): the per-interaction array, which the other states read, regardless"""
        return bool(self._by_env and self.world_size == 1 and self.use_plan
                    and os.environ.get('INVPREF_WEIGHTS_BY_ENV', '1') == '1')

    # ---- what the engine asks (engine.py)
    def _batch_inputs(self, lo: int, hi: int):
        return self.envs[lo:hi], self._sample_weights[lo:hi]

    def _resident(self) -> tuple:
        return self.envs, self._sample_weights

    def _setup_stale(self, moved) -> None:
        if moved is not None and moved[0]:
            self._by_env = False        # (somebody replaced the environments: weights by position until the next stat_envs())
        self._estep_graphs.clear()

    def _before_epochs(self) -> None:
        # per-interaction weights: by environment from the E class weights, or from the N-length array (brought up to date
        # HERE, outside any capture)
        self._epoch_by_env = self._weights_by_env()
        if not self._epoch_by_env:
            self._materialise_sample_weights()

    def _graph_key_extra(self):
        return self._epoch_by_env

    def prepare_graphs(self, run_lengths) -> None:
        super().prepare_graphs(run_lengths)
        # the E-step graphs of both parameter buffers too (their capture warms up and synchronises the host)
        if self.users_tensor.is_cuda and self.world_size == 1:
            for _ in range(2):
                if self._fused_estep_ok():
                    self._estep_state()
                    self._estep_graph(self.cluster_use_random_sort, fused=True, combined=True)
                else:
                    self._estep_graph(self.cluster_use_random_sort)
                if self._fused_seq():
                    self.state.swap()

    # ------------------------------------------------------------------ M-step
    def _coefs(self, alpha):
        return (self.invariant_coe, self.env_aware_coe, self.env_coe, self.L2_coe, self.L1_coe, alpha)

    def _step(self, users, items, scores, envs, weights, alpha, batch_norm: int, losses6=None):
        """one optimiser step on explicit tensors; the six loss terms of this step are ADDED into
        `losses6` (default: state.losses6, zeroed first)."""
        st = self.state
        if losses6 is None:
            losses6 = st.losses6
            losses6.zero_()
        if self._grad_stale:
            # a planned gradient pass (multi-GPU / D > 128 path) OVERWRITES its rows and its Adam does not zero
            # them: the buffer still holds that step's (all-reduced) gradient, and the plan-free kernel below ADDS
            st.grad.zero_()
            self._grad_stale = False
        ops.mstep_grad(st.p_views, st.g_views, users, items, envs, scores, weights, batch_norm, self._coefs(alpha),
                       self._flags, losses6, self.workspace)
        if self.world_size > 1:
            self._all_reduce_step()
        st.step += 1
        self._sched_synced = False
        if self._lazy:      # (the plan-free pass ADDED into an all-zero buffer: only the touched rows and the tail hold anything)
            self._lazy_adam(self._lazy_batch_rows(users, items))
            return
        for o, n in self._adam_ranges:
            ops.adam_(st.param[o:o + n], st.grad[o:o + n], st.exp_avg[o:o + n], st.exp_avg_sq[o:o + n], st.step, self.lr,
                      zero_grad=True)
        if self.world_size > 1:
            if self.exchange == 'scatter':
                st.grad.zero_()             # (only this rank's slice was cleared by its Adam)
            self._exchange_parameters()     # scatter mode: every rank updated its own slice of the flat buffer

    def train_a_batch(self, batch_users_tensor, batch_items_tensor, batch_scores_tensor, batch_envs_tensor,
                      batch_sample_weights, alpha) -> dict:
        """train.py:94-167.  In a sharded run the arguments are this rank's share of the batch (user-sharded:
        the interactions of the users this rank owns)."""
        assert batch_users_tensor.shape == batch_items_tensor.shape == batch_scores_tensor.shape \
            == batch_envs_tensor.shape
        bn = batch_users_tensor.shape[0]
        if self.world_size > 1:
            t = torch.tensor([bn], dtype=torch.int64, device=self.device)
            all_reduce_sum_(t, self.process_group)
            bn = int(t.item())
        dp = self._cached_batch_plan(batch_users_tensor, batch_items_tensor, batch_scores_tensor)
        if dp is not None and self._lazy:
            # lazy Adam: the planned gradient pass over the touched rows only, then Adam on them (a minibatch without a plan:
            # the plan-free pass of _step, which costs what the minibatch touches as it is)
            st = self.state
            st.losses6.zero_()
            st.step += 1
            self._sched_synced = False
            self._gradient_pass(None, planlib.without_streamed_rows(dp), None, None, batch_envs_tensor.contiguous(),
                                batch_scores_tensor.float().contiguous(), batch_sample_weights.contiguous(), bn,
                                self._coefs(alpha), self._flags, st.losses6)
            self._lazy_adam(self._lazy_batch_rows(batch_users_tensor, batch_items_tensor))
        elif dp is not None:
            # the reference's own loop (`for batch in mini_batch(...)`, train.py:204-233) hands over the same slices of
            # the same resident tensors every epoch: from their second sighting they run the planned fused step
            st = self.state
            st.losses6.zero_()
            st.step += 1
            self._sched_synced = False
            ops.mstep_rows_adam(st.p_views, st.p_views_alt, st.m_views, st.v_views, dp, batch_envs_tensor.contiguous(),
                                batch_scores_tensor.float().contiguous(), batch_sample_weights.contiguous(), bn,
                                self._coefs(alpha), self._flags, st.losses6, st.step, self.lr, self.workspace,
                                pure=self._pure)
            st.swap()
            self.planned_batch_steps += 1
        else:
            self._step(batch_users_tensor.contiguous(), batch_items_tensor.contiguous(),
                       batch_scores_tensor.float().contiguous(), batch_envs_tensor.contiguous(),
                       batch_sample_weights.contiguous(), alpha, bn)
        vals = self.state.losses6.tolist()
        return dict(zip(LOSS_KEYS, vals))

    # ------------------------------------------------------------------ the alpha schedule (train.py:214-217)
    def _alpha_for(self, k: int) -> float:
        if self.update_alpha:  # train.py:214-217
            self.alpha = self._scheduled_alpha(self.epoch_cnt, k)
        return self.alpha

    def _scheduled_alpha(self, epoch_cnt: int, k: int) -> float:
        """train.py:214-217 for minibatch k of the epoch that follows `epoch_cnt` completed ones"""
        p = float(k + (epoch_cnt + 1) * self.batch_num) / float((epoch_cnt + 1) * self.batch_num)
        return 2. / (1. + np.exp(-10. * p)) - 1.

    def _alpha_scheduled(self) -> bool:
        return self.update_alpha

    def _sched_alphas(self, j: np.ndarray) -> np.ndarray:
        e1 = (self.epoch_cnt + j // self.batch_num + 1).astype(np.float64) * self.batch_num
        return (2. / (1. + np.exp(-10. * ((j % self.batch_num) + e1) / e1)) - 1.).astype(np.float32)

    def _after_replay(self, n: int) -> None:
        if self.update_alpha:   # what the reference's loop leaves in self.alpha after these epochs
            self.alpha = self._scheduled_alpha(self.epoch_cnt + n - 1, self.batch_num - 1)

    # ------------------------------------------------------------------ E-step
    def _perm_index_dtype(self):
        """the narrowest type that holds E! - 1: what travels to the device per interaction"""
        return np.uint8 if self.envs_num <= 5 else (np.int32 if self.envs_num <= 12 else np.int64)

    def _eps_index(self) -> np.ndarray:
        """train.py:192-196: per batch, np.random.randint picks one of the E! permutations of the eps vector per row --
        the same draws from the same numpy stream as the reference.  Only the INDEX is kept (1 / 4 / 8 bytes per
        interaction); neither the E! x E table of train.py:86-92 nor an N x E table of gathered rows is built: the E-step
        unranks the row on the device (invpref_estep_perm_hip)."""
        parts = []
        for k in range(self.batch_num):
            glen = self.shard.global_batch_len(k)
            idx = np.random.randint(0, self._eps_rows_cnt, glen)  # same numpy stream as the reference
            parts.append(self.shard.select_in_batch(k, idx))
        return np.concatenate(parts).astype(self._perm_index_dtype(), copy=False)

    def _eps_index_device(self, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """the drawn indices on the device, through a pinned staging buffer (a plain asynchronous copy)"""
        idx = self._eps_index()
        cuda = self.device.type == 'cuda'
        stage = getattr(self, '_eps_stage', None)
        if stage is None or stage.numel() != len(idx) or stage.dtype != torch.from_numpy(idx[:0]).dtype:
            stage = self._eps_stage = torch.empty(len(idx), dtype=torch.from_numpy(idx[:0]).dtype, pin_memory=cuda)
            self._eps_stage_done = None
        if self._eps_stage_done is not None:
            self._eps_stage_done.synchronize()    # (the previous E-step's copy has left the staging buffer)
        stage.numpy()[:] = idx
        if out is None:
            out = stage.to(self.device, non_blocking=True)
        else:
            out.copy_(stage, non_blocking=True)
        if cuda:
            self._eps_stage_done = torch.cuda.Event()
            self._eps_stage_done.record()
        return out

    # ---- one GPU: cluster() + stat_envs() are ONE launch (include/invpref_hip.h: invpref_estep_fused_hip) -- the assignment
    # kernel's epilogue folds the counts, cluster()'s diff_num and the class weights; nothing N-long is produced (the M-step
    # looks class_weights[env] up itself) and nothing is cloned behind a replay (results land in a ring the kernel advances)
    def _fused_estep_ok(self) -> bool:
        # (INVPREF_ESTEP_FUSED=0, test hook: the two-launch E-step that sharded runs take, on one GPU)
        return bool(self.world_size == 1 and self.envs.is_cuda and self.use_plan
                    and os.environ.get('INVPREF_ESTEP_FUSED', '1') == '1')

    def _estep_state(self):
        if self._es is None:
            self._es = ops.EstepState(self.envs_num, self.device)
            self._pend_cw = torch.zeros(self.envs_num, dtype=torch.float32, device=self.device)
            self._pend_counts = torch.zeros(self.envs_num, dtype=torch.int64, device=self.device)
        return self._es

    def _issue_fused_estep(self, eps_buf, combined: bool):
        """enqueues (or records, under capture) the fused E-step.  combined: class weights and counts go straight into the
        manager's own tensors (cluster() and stat_envs() called together, train.py:329-330); otherwise into the buffers a later
        stat_envs() applies."""
        es = self._estep_state()
        ops.estep_fused(self.state.p_views, self.users_tensor, self.items_tensor, self.scores_tensor, self.implicit, self.envs,
                        es, self.workspace, perm_index=eps_buf,
                        eps_base=self._eps_base.tolist() if eps_buf is not None else None,
                        counts=self._counts_dev if combined else self._pend_counts,
                        class_weights=self.class_weights if combined else self._pend_cw)

    def _run_fused_estep(self, combined: bool) -> int:
        """one fused E-step on the current stream -- a graph replay where graphs are on -- and the ring row it writes"""
        es = self._estep_state()
        with_eps = self.cluster_use_random_sort
        if self.use_graph and not torch.cuda.is_current_stream_capturing():
            g, eps_buf, _ = self._estep_graph(with_eps, fused=True, combined=combined)
            self._fill_eps(eps_buf)
            g.replay()
            self._eps_replayed(eps_buf)
        else:
            self._issue_fused_estep(self._eps_index_device() if with_eps else None, combined)
        return es.next_row()

    def cluster_and_stat_envs(self, sync: bool = True):
        """cluster() followed by stat_envs() (train.py:329-330: the reference never calls one without the other inside
        train()) -> (diff_num, {env: count}).  sync=False: no read-back; both come back as device views of the E-step ring
        (valid until ops.EstepState.ring_cap further E-steps have run)."""
        if not self._fused_estep_ok():
            return self.cluster(sync=sync), self.stat_envs(sync=sync)
        self.model.eval()
        row = self._run_fused_estep(combined=True)
        self._pending_stat = None
        self._sw_lazy, self._by_env = True, True      # sample_weights == class_weights[envs] from here on, not materialised
        E, ring = self.envs_num, self._es.ring
        if sync:
            vals = ring[row].tolist()
            return int(vals[E]), {env: int(c) for env, c in enumerate(vals[:E])}
        return ring[row, E:E + 1], ring[row, :E]

    def cluster(self, sync: bool = True):
        """train.py:235-259.  sync=False: no read-back, returns diff_num as a device int64[1] tensor."""
        self.model.eval()
        if self._fused_estep_ok() and not torch.cuda.is_current_stream_capturing():
            # cluster() WITHOUT the stat_envs() that follows it in train(): the reference's sample_weights keep their values BY
            # POSITION (train.py:67, :278) while the environments move -- bring the array up to date with the old environments
            # first, and read it per interaction until stat_envs() runs
            self._materialise_sample_weights()
            row = self._run_fused_estep(combined=False)
            self._by_env = False
            self._pending_stat = 'fused'
            diff = self._es.ring[row, self.envs_num:self.envs_num + 1]
            return int(diff.item()) if sync else diff
        if self.world_size == 1 and self.use_graph and self.envs.is_cuda and not torch.cuda.is_current_stream_capturing():
            # one HIP-graph replay instead of a handful of eager launches behind the Python operator layer (the
            # host-side cost of those was several times the 40 us the kernels take); the permutation indices of
            # train.py:192-196 are host random numbers: they are copied into the buffer the graph reads
            self._materialise_sample_weights()
            counts, diff, cw, sw = self._cluster_replay(self.cluster_use_random_sort)
            self._pending_stat = (counts, cw, sw)
            self._by_env = False
            return int(diff.item()) if sync else diff.clone()
        perm = self._eps_index_device() if self.cluster_use_random_sort else None
        self._materialise_sample_weights()
        self._by_env = False
        # new assignments overwrite self.envs in place (the kernel reads old_envs[i] before writing i)
        new, counts, diff, cw, sw = ops.estep(self.state.p_views, self.users_tensor, self.items_tensor,
                                              self.scores_tensor, self.implicit, self.envs, self.workspace,
                                              new_envs=self.envs, want_weights=(self.world_size == 1),
                                              perm_index=perm, eps_base=self._eps_base.tolist() if perm is not None else None)
        if self.world_size > 1:
            cd = torch.cat([counts, diff])
            all_reduce_sum_(cd, self.process_group)
            counts, diff = cd[:-1].contiguous(), cd[-1:]
            cw, sw = ops.sample_weights(self.envs, counts, self.n_total, self.envs_num)
        self._pending_stat = (counts, cw, sw)
        return int(diff.item()) if sync else diff.clone()

    def _estep_graph(self, with_eps: bool, fused: bool = False, combined: bool = True):
        """The captured E-step for the CURRENT parameter buffer and interaction arrays, captured on first use: (graph, eps
        staging buffer or None, output tensors in the graph's pool -- None for the fused form, whose outputs are the manager's
        own tensors and the ring).  The capture needs a warm-up E-step and a host sync; prepare_graphs() does it ahead of time
        for both parameter buffers, so that an E-step inside a timed loop only replays."""
        key = (self.state.p_views[0].data_ptr(), self.envs.data_ptr(), self.users_tensor.data_ptr(), with_eps, fused, combined)
        ent = self._estep_graphs.get(key)
        if ent is None:
            # (the buffer the captured E-step reads its permutation indices from, 1 / 4 / 8 bytes per interaction: up to
            #  seven environments PINNED HOST memory the kernel reads in place -- no copy in front of the replay --
            #  otherwise a device buffer the staging buffer is copied into)
            eps_buf = None
            if with_eps:
                dt = torch.from_numpy(np.zeros(0, self._perm_index_dtype())).dtype
                n_loc = self.users_tensor.shape[0]
                # (test hook INVPREF_EPS_PINNED=0: the device buffer that eight or more environments take anyway, at any E.
                #  A copy on a side stream, ahead of the replay, was measured slower: the bench's interval 80 us longer)
                pinned = self.envs_num <= 7 and os.environ.get('INVPREF_EPS_PINNED', '1') == '1'
                eps_buf = torch.zeros(n_loc, dtype=dt, pin_memory=True) if pinned \
                    else torch.zeros(n_loc, dtype=dt, device=self.device)

            def run():
                if fused:
                    self._issue_fused_estep(eps_buf, combined)
                    return None
                _, counts, diff, cw, sw = ops.estep(self.state.p_views, self.users_tensor, self.items_tensor,
                                                    self.scores_tensor, self.implicit, self.envs, self.workspace,
                                                    new_envs=self.envs, want_weights=True, perm_index=eps_buf,
                                                    eps_base=self._eps_base.tolist() if with_eps else None)
                return counts, diff, cw, sw
            # sizes the workspace outside the capture; the warm-up is not an E-step: the environments, the class weights, the
            # counts and the ring position are put back
            keep = self.envs.clone()
            keep_cw, keep_c = self.class_weights.clone(), self._counts_dev.clone()
            run()
            self.envs.copy_(keep)
            if fused:
                self.class_weights.copy_(keep_cw)
                self._counts_dev.copy_(keep_c)
                self._es.state[1] -= 1
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with _gc_paused(), torch.cuda.graph(g):
                outs = run()
            ent = self._estep_graphs[key] = (g, eps_buf, outs)
        return ent

    def _fill_eps(self, eps_buf):
        """this E-step's permutation indices (host numpy stream, like the reference) into the buffer the graph reads"""
        if eps_buf is not None and not eps_buf.is_cuda:
            done = getattr(self, '_eps_read_done', None)
            if done is not None:
                done.synchronize()                 # (the previous replay has read the buffer)
            eps_buf.numpy()[:] = self._eps_index()
        elif eps_buf is not None:
            self._eps_index_device(out=eps_buf)

    def _eps_replayed(self, eps_buf):
        if eps_buf is not None and not eps_buf.is_cuda:
            self._eps_read_done = torch.cuda.Event()
            self._eps_read_done.record()

    def _cluster_replay(self, with_eps: bool):
        """One graph per parameter buffer (the fused M-step ping-pongs between two) and per interaction-array set."""
        g, eps_buf, outs = self._estep_graph(with_eps)
        self._fill_eps(eps_buf)
        g.replay()
        self._eps_replayed(eps_buf)
        return outs

    def cluster_a_batch(self, batch_users_tensor, batch_items_tensor, batch_scores_tensor) -> torch.Tensor:
        """train.py:169-202 for one batch (single-rank semantics)."""
        perm = None
        if self.cluster_use_random_sort:
            idx = np.random.randint(0, self._eps_rows_cnt, batch_users_tensor.shape[0])
            perm = torch.from_numpy(idx.astype(self._perm_index_dtype(), copy=False)).to(self.device)
        new, _, _, _, _ = ops.estep(self.state.p_views, batch_users_tensor.contiguous(),
                                    batch_items_tensor.contiguous(), batch_scores_tensor.float().contiguous(),
                                    self.implicit, None, self.workspace, want_weights=False, perm_index=perm,
                                    eps_base=self._eps_base.tolist() if perm is not None else None)
        return new

    def stat_envs(self, sync: bool = True):
        """train.py:268-280.  sync=False: no read-back, returns the per-env counts as a device tensor."""
        pend = getattr(self, '_pending_stat', None)
        self._pending_stat = None
        lazy_ok = self._fused_estep_ok()
        if isinstance(pend, str):                  # a fused cluster() ran: its epilogue left counts and class weights behind
            counts, cw, sw = self._pend_counts, self._pend_cw, None
        elif pend is not None:
            counts, cw, sw = pend
        elif self.world_size == 1:
            counts, cw, sw = ops.stat_envs(self.envs, self.envs_num, self.workspace, want_sample_weights=not lazy_ok)
        else:
            counts, _, _ = ops.stat_envs(self.envs, self.envs_num, self.workspace, want_sample_weights=False)
            all_reduce_sum_(counts, self.process_group)
            cw, sw = ops.sample_weights(self.envs, counts, self.n_total, self.envs_num)
        # in place: the epoch loop (and a captured HIP graph of it) holds pointers into these buffers
        self.class_weights.copy_(cw)
        if lazy_ok:
            # one GPU: the planned M-step takes class_weights[env] (INVPREF_WEIGHTS_BY_ENV); the N-length array is
            # materialised only if somebody asks for the attribute
            self._counts_dev.copy_(counts)
            self._sw_lazy, self._by_env = True, True
        else:
            if sw is None:
                _, sw = ops.sample_weights(self.envs, counts, self.n_total, self.envs_num)
            self._sample_weights.copy_(sw)
            self._sw_lazy = False
            self._by_env = True      # (consistent; whether launches USE it: _weights_by_env())
        return {env: int(c) for env, c in enumerate(counts.tolist())} if sync else counts.clone()

    def update_each_env_count(self):  # train.py:261-266
        counts, _, _ = ops.stat_envs(self.envs, self.envs_num, self.workspace, want_sample_weights=False)
        if self.world_size > 1:
            all_reduce_sum_(counts, self.process_group)
        self.each_env_count.update({e: c for e, c in enumerate(counts)})

    # ------------------------------------------------------------------ outer loop (train.py:282-342)
    # The engine's loop (evaluations and runs of epochs) with the cluster events as its hooks; their records are kept here.
    def _ends_run(self, e: int) -> bool:
        return e % self.cluster_interval == 0

    def _after_first_evaluation(self) -> None:
        self.stat_envs()        # train.py:292-301

    def _after_run_events(self, defer: bool) -> None:
        if (self.epoch_cnt % self.cluster_interval) != 0:
            return
        ev = self._cluster_events
        if (self.begin_cluster_epoch is None or self.begin_cluster_epoch <= self.epoch_cnt) \
                and (self.stop_cluster_epoch is None or self.stop_cluster_epoch > self.epoch_cnt):
            diff_num, envs_cnt = self.cluster_and_stat_envs(sync=not defer)   # train.py:329-330, one launch
        else:
            diff_num, envs_cnt = 0, self.stat_envs(sync=not defer)
        ev['diff_num'].append(diff_num)
        if defer and self._es is not None and len(ev['diff_num']) % (self._es.ring_cap - 8) == 0:
            # (deferred results are views of the E-step ring: read them out before it wraps)
            ev['diff_num'] = [int(d.item()) if torch.is_tensor(d) else d for d in ev['diff_num']]
            ev['envs_cnt'] = [t.tolist() if torch.is_tensor(t) else t for t in ev['envs_cnt']]
            envs_cnt = envs_cnt.tolist()
        ev['epoch'].append(self.epoch_cnt)
        ev['envs_cnt'].append(envs_cnt)
        if not defer:
            print('cluster at epoch:', self.epoch_cnt)
            print('diff num:', diff_num)
            print(transfer_loss_dict_to_line_str(envs_cnt))

    def _train_span(self, silent: bool, auto: bool, initial: bool):
        """The engine's two result tuples and (diff_num per cluster event, env counts, epochs); nothing of the events is read
        back inside a silent / auto loop (their results stay on the device until the end)."""
        self._cluster_events = dict(diff_num=[], envs_cnt=[], epoch=[])
        losses, tests = super()._train_span(silent, auto, initial)
        ev, self._cluster_events = self._cluster_events, None
        if silent or auto:      # the loop deferred its read-backs: here is the events' share of the one at the end
            ev['diff_num'] = [int(d.item()) if torch.is_tensor(d) else d for d in ev['diff_num']]
            ev['envs_cnt'] = [{env: int(c) for env, c in enumerate(t.tolist() if torch.is_tensor(t) else t)}
                              for t in ev['envs_cnt']]
        return losses, tests, (ev['diff_num'], ev['envs_cnt'], ev['epoch'])


def _unrank_permutations(idx: np.ndarray, base: np.ndarray) -> np.ndarray:
    """Row idx[i] of ``list(itertools.permutations(base))`` (lexicographic in positions), without
    building the E! table (the reference builds it eagerly, train.py:86-92, and cannot be
    constructed for E >= 11)."""
    E = len(base)
    idx = np.asarray(idx, dtype=np.int64).copy()
    n = len(idx)
    out = np.empty((n, E), np.float32)
    avail = np.tile(np.arange(E, dtype=np.int64), (n, 1))
    for pos in range(E):
        f = math.factorial(E - 1 - pos)
        d = idx // f
        idx = idx % f
        pick = avail[np.arange(n), d]
        out[:, pos] = base[pick]
        # remove the picked element from each row's availability list
        keep = np.ones_like(avail, dtype=bool)
        keep[np.arange(n), d] = False
        avail = avail[keep].reshape(n, -1)
    return out


class ImplicitTrainManager(_InvPrefTrainManager):
    """reference train.py:16-342 (BCELoss)."""
    implicit = True


class ExplicitTrainManager(_InvPrefTrainManager):
    """reference train.py:693-1019 (MSELoss)."""
    implicit = False


class ImplicitTrainStaticPopularityManager(ImplicitTrainManager):
    """reference train.py:484-690: ImplicitTrainManager + per-environment popularity statistics every
    `static_pop_interval` epochs.  The statistics are one device pass over the resident interactions
    (`invpref_static_pop_hip`) instead of numpy boolean masks per environment.  Single GPU."""

    def __init__(self, model, evaluator, device, data_loader, training_data, batch_size, epochs, cluster_interval,
                 evaluate_interval, lr, invariant_coe, env_aware_coe, env_coe, L2_coe, L1_coe, static_pop_interval,
                 alpha=None, use_class_re_weight=False, test_begin_epoch=0, begin_cluster_epoch=None,
                 stop_cluster_epoch=None, cluster_use_random_sort=True, use_recommend_re_weight=True):
        super().__init__(model=model, evaluator=evaluator, device=device, training_data=training_data,
                         batch_size=batch_size, epochs=epochs, cluster_interval=cluster_interval,
                         evaluate_interval=evaluate_interval, lr=lr, invariant_coe=invariant_coe,
                         env_aware_coe=env_aware_coe, env_coe=env_coe, L2_coe=L2_coe, L1_coe=L1_coe, alpha=alpha,
                         use_class_re_weight=use_class_re_weight, test_begin_epoch=test_begin_epoch,
                         begin_cluster_epoch=begin_cluster_epoch, stop_cluster_epoch=stop_cluster_epoch,
                         cluster_use_random_sort=cluster_use_random_sort,
                         use_recommend_re_weight=use_recommend_re_weight, rank=0, world_size=1)
        self.training_np = training_data.cpu().numpy()
        self.static_pop_interval = static_pop_interval
        self.data_loader = data_loader
        dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(self.device)  # noqa: E731
        self._pop_tabs = (dev(data_loader.user_inter_cnt_np, np.int64), dev(data_loader.item_inter_cnt_np, np.int64),
                          dev(data_loader.user_inter_cnt_normalize_np, np.float64),
                          dev(data_loader.item_inter_cnt_normalize_np, np.float64))

    def static_pop(self) -> dict:
        """train.py:509-571: {statistic: {env: mean}}."""
        out = ops.static_pop(self.users_tensor, self.items_tensor, self.envs, self.envs_num, *self._pop_tabs,
                             self.workspace).tolist()
        return {key: {env: out[env][j] for env in range(self.envs_num)} for j, key in enumerate(ops.POP_KEYS)}

    def final_cluster_stat(self, colors_list: list):
        """train.py:573-601: per-interaction popularity values grouped by environment, for the scatter plot."""
        assert len(colors_list) == self.envs_num
        envs = self.envs.cpu().numpy()
        order = np.argsort(envs, kind='stable')           # env 0 rows first, original order inside an env
        u, i = self.training_np[order, 0], self.training_np[order, 1]
        dl = self.data_loader
        colors = [colors_list[e] for e in envs[order].tolist()]
        return (dl.query_users_inter_cnt(u).tolist(), dl.query_items_inter_cnt(i).tolist(),
                dl.query_users_inter_cnt_normalize(u).tolist(), dl.query_items_inter_cnt_normalize(i).tolist(), colors)

    def train(self, silent: bool = False, auto: bool = False):
        """train.py:603-690: the InvPref loop + `static_pop` every static_pop_interval epochs; a fourth result tuple."""
        import json
        stat_dicts, stat_epochs = [], []
        epochs_total = self.epochs
        loss_l, loss_e, test_l, test_e, diff_l, cnt_l, cl_e = [], [], [], [], [], [], []
        first = True
        while first or self.epoch_cnt < epochs_total:
            # run the base loop up to the next statistics epoch (it evaluates at its start only the first time)
            nxt = min(epochs_total, (self.epoch_cnt // self.static_pop_interval + 1) * self.static_pop_interval)
            self.epochs = nxt
            (l, le), (t, te), (d, c, ce) = self._train_span(silent, auto, initial=first)
            first = False
            loss_l += l; loss_e += le; test_l += t; test_e += te; diff_l += d; cnt_l += c; cl_e += ce
            if self.epoch_cnt % self.static_pop_interval == 0 and self.epoch_cnt > 0:
                pop = self.static_pop()
                stat_epochs.append(self.epoch_cnt)
                stat_dicts.append(pop)
                if not silent and not auto:
                    print('pop stat at epoch:', self.epoch_cnt)
                    print(json.dumps(pop, indent=4))
            if self.epoch_cnt >= epochs_total:
                break
        self.epochs = epochs_total
        merged = {key: {env: [d[key][env] for d in stat_dicts] for env in stat_dicts[0][key]} for key in stat_dicts[0]} \
            if stat_dicts else {}
        return (loss_l, loss_e), (test_l, test_e), (diff_l, cnt_l, cl_e), (merged, stat_epochs)
