"""The epoch engine the minibatch train managers are built on, ``_EpochEngine``, and the outer loop under it, ``_OuterLoop``.

It owns what a run of optimiser steps over STATIC minibatches needs and nothing about what the steps mean: this rank's share
of the interactions, the flat parameter / gradient / moment buffers (``FlatState``), the row plans, the per-minibatch
arguments (``RawBatch``), the fused, unfused, alternating and lazy step sequences, the device-side Adam schedule, whole-epoch
HIP graphs, the sharded exchanges and ``train_epochs()``.  train(), the evaluate-and-epochs loop around train_epochs(), is
``_OuterLoop``'s: the managers that are not epoch-engine managers (baseline.py: ALS, EASE, Mult-DAE) derive from that alone.

A manager derives from it and answers a few questions through methods the engine calls (DESIGN.md §4.6 lists them); every
default is the answer of a plain PureMF step.  ``train._InvPrefTrainManager`` adds the environments, their weights, the
E-step and the alpha schedule that way; ``baseline._BasicTrainManager`` adds next to nothing.
"""
from __future__ import annotations

import contextlib
import gc
import math
import os
import time
from typing import NamedTuple, Optional

import numpy as np
import torch

import ctypes as C

from . import _capi, ops
from . import plan as planlib
from .parallel import (RowShard, UserShard, all_gather_chunks_, all_reduce_min_, all_reduce_sum_,
                       reduce_scatter_sum_)

LOSS_KEYS = ('invariant_loss', 'env_aware_loss', 'envs_loss', 'L2_reg', 'L1_reg', 'loss')
_ALIGN = 64  # floats; every table starts on a 256-byte boundary of the flat buffer


def transfer_loss_dict_to_line_str(d: dict) -> str:
    return ', '.join(f'{k}: {v}' for k, v in d.items())  # utils.py:254-260


@contextlib.contextmanager
def _gc_paused():
    """No cyclic garbage collection inside a stream capture.  torch.cuda.graph no longer collects on entry, so a collection
    that falls into the capture may run the destructor of an unrelated dead object that owns a graph, an event or pinned
    memory: calls a capturing thread must not make (seen as an abort of the process).  It runs after the capture instead."""
    was = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was:
            gc.enable()


def touched_row_offsets(users, items, offsets, user_tabs, item_tabs, D: int):
    """First float, in the flat buffers, of every row of the user and item tables that a minibatch touches: the sorted unique
    `offsets[table] + id * D` over the ids in `users` (tables `user_tabs`) and `items` (tables `item_tabs`).  numpy arrays give
    an int64 numpy array (the static minibatches, listed once on the host); tensors an int64 tensor on their device
    (caller-supplied minibatches: torch.unique there).  Tables do not overlap, so neither do the rows: what the packed
    exchange copies and lazy Adam updates."""
    if isinstance(users, np.ndarray):
        tu, ti = np.unique(users.astype(np.int64, copy=False)), np.unique(items.astype(np.int64, copy=False))
        parts = [offsets[i] + tu * D for i in user_tabs] + [offsets[i] + ti * D for i in item_tabs]
        return np.sort(np.concatenate(parts)).astype(np.int64)
    tu, ti = torch.unique(users.reshape(-1).long()), torch.unique(items.reshape(-1).long())
    parts = [offsets[i] + tu * D for i in user_tabs] + [offsets[i] + ti * D for i in item_tabs]
    return torch.sort(torch.cat(parts)).values.contiguous()


class FlatState:
    """params / grads / exp_avg / exp_avg_sq as four flat buffers + per-table views."""

    def __init__(self, tabs, device, order=None, chunks: int = 1):
        """tabs: the model's parameter tensors (InvPref: the seven of state_dict order; PureMF: two).
        order: physical placement of the tables inside the flat buffers (default: as listed).  A user-sharded
        run puts the two user tables first, so that everything the ranks share is ONE contiguous range.
        chunks: the buffers' capacity `cap` is padded so that it splits into that many equal pieces of whole
        256-byte lines (the reduce-scatter / all-gather exchange of a row-sharded run); `n` stays the used length."""
        tabs = list(tabs)
        self.shapes = [tuple(p.shape) for p in tabs]
        self.offsets = [0] * len(tabs)
        off = 0
        for i in (range(len(tabs)) if order is None else order):
            self.offsets[i] = off
            off += (tabs[i].numel() + _ALIGN - 1) // _ALIGN * _ALIGN
        self.n = off
        piece = max(1, chunks) * _ALIGN
        self.cap = cap = (off + piece - 1) // piece * piece
        self.param_full = torch.zeros(cap, dtype=torch.float32, device=device)
        self.param = self.param_full[:self.n]
        # +8: the six loss partials ride at the tail of the gradient buffer so that ONE all-reduce
        # carries everything; they sit behind the padding: [0, n) gradient, [cap, cap + 6) losses
        self.grad_full = torch.zeros(cap + 8, dtype=torch.float32, device=device)
        self.grad_ext = self.grad_full          # gradient | padding (zeros) | loss tail: one contiguous range
        self.grad = self.grad_full[:self.n]
        self.losses6 = self.grad_full[cap:cap + 6]
        self.exp_avg = torch.zeros(self.n, dtype=torch.float32, device=device)
        self.exp_avg_sq = torch.zeros(self.n, dtype=torch.float32, device=device)
        # double buffer for the fused M-step+Adam pass (reads old rows, writes new rows)
        self.param_alt = torch.zeros(self.n, dtype=torch.float32, device=device)
        self.p_views = self._views(self.param)
        self.p_views_alt = self._views(self.param_alt)
        self.g_views = self._views(self.grad)
        self.m_views = self._views(self.exp_avg)
        self.v_views = self._views(self.exp_avg_sq)
        self._tabs = tabs
        with torch.no_grad():
            for p, view in zip(tabs, self.p_views):
                view.copy_(p.detach().to(device=device, dtype=torch.float32))
                p.data = view  # the module's parameters now alias the flat buffer
        self.step = 0

    def swap(self):
        """the fused pass wrote the new parameters into the alternate buffer: make it current and
        re-point the module's parameters at it (metadata only, no copy)."""
        self.param, self.param_alt = self.param_alt, self.param
        self.p_views, self.p_views_alt = self.p_views_alt, self.p_views
        for p, view in zip(self._tabs, self.p_views):
            p.data = view

    def _views(self, flat):
        return [flat[o:o + int(np.prod(s))].view(s) for o, s in zip(self.offsets, self.shapes)]


class RawBatch(NamedTuple):
    """one static minibatch as the epochs' launches read it: views of this rank's resident arrays"""
    lo: int                             # first local row
    n: int                              # local rows
    global_n: int                       # rows of the GLOBAL minibatch: the denominator of every mean()
    users: torch.Tensor
    items: torch.Tensor
    scores: torch.Tensor
    envs: Optional[torch.Tensor]        # None: PureMF
    weights: Optional[torch.Tensor]     # InvPref: the slice of sample_weights; PureMF: _pure_weights() or None

    @property
    def env_ids(self):
        """`envs` as the engine reads it: a per-interaction argument of the step's kernels, whatever its manager keeps there"""
        return self.envs


class _OuterLoop:
    """train(): the outer loop of every manager (train.py:428-461; InvPref's: :282-342) -- the evaluation in front of the first
    epoch, runs of epochs up to the next evaluation or event enqueued together, the records, the printed lines, and ONE
    read-back at the end when nothing is printed.  It knows nothing about what an epoch is.  A manager supplies
        epoch_cnt, epochs, evaluate_interval, test_begin_epoch, evaluator
        train_epochs(n, sync)   n epochs enqueued, epoch_cnt moved on: their loss dicts (sync), else a device tensor with one
                                row per epoch, which read_back() takes later
        _LOSS_KEYS              the names of a row's leading values
    and may override the hooks below, each of which does nothing by default."""
    _LOSS_KEYS = ()

    @classmethod
    def loss_dicts(cls, dev_losses: torch.Tensor) -> list:
        """the loss dicts of a device tensor [n, terms] (or [terms]): _LOSS_KEYS over each row's leading values"""
        return [dict(zip(cls._LOSS_KEYS, v)) for v in dev_losses.reshape(-1, dev_losses.shape[-1]).tolist()]

    def read_back(self, dev_losses: torch.Tensor) -> list:
        """what the deferred loop reads at its end: loss_dicts, behind whatever check the manager makes at a read-back"""
        return self.loss_dicts(dev_losses)

    def _before_run(self) -> None:
        """enqueued in front of every run of epochs (baseline.py: ExpoMFTrainManager)"""

    def _after_run(self) -> None:
        """enqueued behind every run of epochs, before its records are taken"""

    def _ends_run(self, e: int) -> bool:
        """does an event of the manager's own follow epoch e?  (the run of epochs ends there)"""
        return False

    def _before_evaluation(self) -> None:
        """in front of every evaluation: the model is brought to where the evaluator reads it"""

    def _after_first_evaluation(self) -> None:
        """behind the evaluation in front of the first epoch"""

    def _after_run_events(self, defer: bool) -> None:
        """behind every run of epochs and its evaluation, where _ends_run() or another event ended it; defer: read nothing back
        (results are collected by the manager's own _train_span)"""

    def _after_training(self) -> None:
        """behind the last run, in front of the deferred read-back: a manager's sticky errors raise here"""

    def _epochs_to_next_event(self) -> int:
        """How many epochs train() may enqueue before the next evaluation, event of the manager's own or end of training."""
        r = 1
        while r < 64:
            e = self.epoch_cnt + r
            if e >= self.epochs or self._ends_run(e) \
                    or (e % self.evaluate_interval == 0 and e >= self.test_begin_epoch):
                break
            r += 1
        return r

    def train(self, silent: bool = False, auto: bool = False):
        """((loss dicts, epochs), (test results, epochs)) of the outer loop"""
        return self._train_span(silent, auto, initial=True)

    def _train_span(self, silent: bool, auto: bool, initial: bool):
        """The outer loop from the current epoch up to self.epochs; `initial` runs the epoch-0 evaluation (and what the
        manager does behind it) first."""
        test_result_list, test_epoch_list = [], []
        loss_result_list, train_epoch_index_list = [], []
        # nothing printed -> nothing is read back inside the loop (losses, the results of the manager's own events and -- from
        # an evaluator with evaluate_async -- the evaluations stay on the device until the end): the GPU never waits for the
        # host between epochs, events and evaluations.  An evaluator without evaluate_async is called synchronously.
        defer = bool(silent or auto)
        evaluate = getattr(self.evaluator, 'evaluate_async', None) if defer else None
        pending = evaluate is not None
        evaluate = evaluate or self.evaluator.evaluate

        def test():
            self._before_evaluation()
            result = evaluate()
            test_result_list.append(result)
            test_epoch_list.append(self.epoch_cnt)
            return result

        def show_test(result) -> None:
            if not defer:
                print('test at epoch:', self.epoch_cnt)
                print(transfer_loss_dict_to_line_str(result))

        if initial:
            result = test()
            self._after_first_evaluation()
            show_test(result)

        while self.epoch_cnt < self.epochs:
            # the epochs up to the next evaluation or event are enqueued together (one read-back);
            # the records and the printed lines are the same, in the same order, as one epoch at a time
            first = self.epoch_cnt + 1
            self._before_run()
            run = self.train_epochs(self._epochs_to_next_event(), sync=not defer)
            self._after_run()
            for i in range(len(run)):
                train_epoch_index_list.append(first + i)
                loss_result_list.append(run[i])
                if not defer:
                    print('train epoch:', first + i)
                    if run[i]:      # (a closed form has no loss to report: its dict is empty, and gets no line)
                        print(transfer_loss_dict_to_line_str(run[i]))

            if (self.epoch_cnt % self.evaluate_interval) == 0 and self.epoch_cnt >= self.test_begin_epoch:
                show_test(test())

            self._after_run_events(defer)

        self._after_training()
        if defer:  # one read-back for everything
            loss_result_list = self.read_back(torch.stack(loss_result_list)) if loss_result_list else []
            if pending:
                test_result_list = [p.result() for p in test_result_list]

        return (loss_result_list, train_epoch_index_list), (test_result_list, test_epoch_list)


class _EpochEngine(_OuterLoop):
    """See the module's docstring.  What a manager may override, each default being plain PureMF's answer: _batch_inputs,
    _resident, _setup_stale, _before_epochs, _step_weights, _graph_key_extra, _alpha_for, _alpha_scheduled, _sched_alphas,
    _after_replay, _env_count; and, as before, _coefs, _pure_weights, _gradient_pass, _after_gradient_pass; and the hooks of
    _OuterLoop."""
    _LOSS_KEYS = LOSS_KEYS
    implicit = True
    _lazy_adam_unsupported = None       # a manager that cannot run lazy Adam names the reason here (set_lazy_adam)
    _pure = True                        # the step's kernel form: PureMF's two tables (False: InvPref's seven)
    _make_tables = staticmethod(_capi.make_pure_tables)
    _env_count = 0                      # what the row-plan builders take as env_num (InvPref: its number of environments)
    alpha = 0.                          # the last coefficient of _coefs(): constant unless a manager schedules it (_alpha_for)

    def _coefs(self, alpha):
        """the six coefficients of the step's loss (ops.mstep_*), `alpha` being _alpha_for()'s value for the minibatch"""
        raise NotImplementedError

    def _init_engine(self, model, evaluator, device, training_data: torch.Tensor, batch_size: int, epochs: int,
                     evaluate_interval: int, lr: float, L2_coe: float, L1_coe: float, test_begin_epoch: int, rank, world_size,
                     process_group, *, flags: int, users_first, env_switches: bool):
        """What every manager's constructor does (the PureMF managers of baseline.py included): this rank's share of the
        interactions, the flat state and the bookkeeping of the plan, graph, schedule and alternating machinery.
        flags: the step's INVPREF_* flags on rank 0 (the dense regulariser is added once: the other ranks drop DENSE_REG);
        users_first: the tables' placement in the flat buffers of a user-sharded run (None: as listed);
        env_switches: honour INVPREF_NO_PLAN / INVPREF_UNFUSED (the PureMF managers always take the planned fused step)."""
        if model.implicit != self.implicit:
            raise TypeError(f'{type(self).__name__} needs an {"implicit" if self.implicit else "explicit"} model')
        self.model = model
        self.evaluator = evaluator
        self.device = torch.device(device)
        self.process_group = process_group
        if world_size is None:
            import torch.distributed as dist
            world_size = dist.get_world_size(process_group) if dist.is_available() and dist.is_initialized() else 1
            rank = dist.get_rank(process_group) if world_size > 1 else 0
        self.rank, self.world_size = int(rank or 0), int(world_size)

        n_total = training_data.shape[0]
        self.n_total = n_total
        self.batch_size = batch_size
        self.batch_num = math.ceil(n_total / batch_size)
        # multi-GPU: the literal row split of SURVEY 8(e) / north_star by default (parallel.RowShard, parameters replicated);
        # INVPREF_SHARD=users partitions the users instead (parallel.UserShard: only the item-side gradient is all-reduced;
        # bench.py sets the variable)
        # (testing aid INVPREF_FORCE_SHARDED_PATH=1: the sharded step sequence -- gradient pass -> all-reduce -> stand-alone
        #  Adam --, either layout, on one rank)
        self._force_sharded_path = os.environ.get('INVPREF_FORCE_SHARDED_PATH', '0') == '1'
        self.shard_mode = os.environ.get('INVPREF_SHARD', 'rows') if (self.world_size > 1 or self._force_sharded_path) else 'rows'
        if self.shard_mode not in ('users', 'rows'):
            raise ValueError('INVPREF_SHARD must be "users" or "rows"')
        if self.shard_mode == 'users':
            self.shard = UserShard(training_data[:, 0].cpu().numpy(), n_total, batch_size, model.user_num, self.rank,
                                   self.world_size)
        else:
            self.shard = RowShard(n_total, batch_size, self.rank, self.world_size)
        td = training_data
        if self.world_size > 1:
            td = training_data.index_select(0, self.shard.local_rows().to(training_data.device))
        # the reference's attribute names, holding this rank's rows: what the kernels read
        self.users_tensor = td[:, 0].contiguous().to(self.device)
        self.items_tensor = td[:, 1].contiguous().to(self.device)
        self.scores_tensor = td[:, 2].float().contiguous().to(self.device)

        self.evaluate_interval, self.epochs = evaluate_interval, epochs
        self.lr = lr
        self.L2_coe, self.L1_coe = L2_coe, L1_coe
        self.epoch_cnt = 0
        self.test_begin_epoch = test_begin_epoch

        self.model.to(self.device)
        # row-sharded exchange (INVPREF_EXCHANGE; bench.py sets it): "scatter" = reduce-scatter of the flat gradient, Adam on
        # this rank's 1/G slice of the flat buffers, all-gather of the new parameters (same bytes on the wire as the
        # all-reduce, the dense Adam stream cut G-fold); "allreduce" = SURVEY 8(e) as written: every rank reduces and updates everything; "packed" =
        # the all-reduce over the rows the GLOBAL minibatch touches only (+ the small tables): every other gradient row is
        # zero on every rank, so nothing else needs the wire (_setup_packed)
        self.exchange = os.environ.get('INVPREF_EXCHANGE', 'allreduce') if self.shard_mode == 'rows' else 'allreduce'
        if self.exchange not in ('scatter', 'allreduce', 'packed'):
            raise ValueError('INVPREF_EXCHANGE must be "scatter", "allreduce" or "packed"')
        self.state = FlatState(model.tables(), self.device, order=users_first if self.shard_mode == 'users' else None,
                               chunks=self.world_size if self.exchange == 'scatter' else 1)
        self._setup_ranges(model)
        if self.exchange == 'packed':
            self._setup_packed(training_data[:, 0], training_data[:, 1])
        self.workspace = ops.Workspace(self.device)
        self._flags = flags if self.rank == 0 else flags & ~_capi.DENSE_REG
        # atomic-free planned M-step (plan.py) unless INVPREF_NO_PLAN=1 (then: float-atomic scatter-add, the path of
        # train_a_batch on minibatches without a plan -- the test hook that runs it for whole epochs)
        self.use_plan = not (env_switches and os.environ.get('INVPREF_NO_PLAN', '0') == '1')
        # (measured, tools/kbench.py, planned fused step vs plan-free gradient + Adam: Yahoo class 19 vs 78 us,
        #  MovieLens class -- E = 8, D = 128, 65 536 interactions -- 110 vs 181 us, MIND class -- E = 16, D = 256,
        #  262 144 interactions -- 1.1 vs 1.66 ms: the plan wins everywhere, so it is the default for every shape)
        # INVPREF_UNFUSED=1: gradient pass + flat Adam kernel instead of the fused pass on one GPU (the sequence a sharded
        # rank runs, without the exchange); every row length takes the fused pass by default
        self._unfused = env_switches and self.use_plan and os.environ.get('INVPREF_UNFUSED', '') == '1'
        self._plans = None
        self._batch_plans, self.planned_batch_steps = {}, 0   # train_a_batch on caller tensors: see _cached_batch_plan
        self._batch_plans_foreign = {}
        # runs of whole epochs as one HIP graph launch (single GPU, planned path); INVPREF_NO_GRAPH=1 disables (test hook:
        # the eager launches that sharded runs and single calls take, against the replay)
        self.use_graph = os.environ.get('INVPREF_NO_GRAPH', '0') != '1'
        import torch.distributed as _dist
        self._collective_ok = _dist.is_available() and _dist.is_initialized()
        self._graphs, self._graph_warm = {}, False
        self._grad_stale = False
        self._sched = None
        self._sched_synced = False
        self._alt = None
        self._lazy = False           # set_lazy_adam()
        self._alt_parked = None      # the alternating form's plans and workspace while lazy Adam is on
        self._lazy_consts = None     # the tail of small tensors, the tables' roles and alignment (set_lazy_adam)
        self._lazy_state = None      # the row lists and plans of the static minibatches under lazy Adam (_lazy_setup)

    def _pure_weights(self, lo: int, hi: int):
        """PureMF managers: the per-interaction weights of the local rows [lo, hi) that the epochs' launches read under
        INVPREF_REWEIGHT_REC (the IPS / SNIPS managers of baseline.py), or None (plain PureMF)"""
        return None

    # ---- what a manager with per-interaction state of its own answers (train.py: _InvPrefTrainManager)
    def _batch_inputs(self, lo: int, hi: int):
        """(RawBatch.envs, RawBatch.weights) of the local rows [lo, hi): views of resident tensors, taken once by _raw_setup"""
        return None, self._pure_weights(lo, hi)

    def _resident(self) -> tuple:
        """the resident tensors _batch_inputs() slices that somebody may REPLACE between two runs of epochs: a new address
        makes the raw setup stale (the interaction arrays themselves are never replaced)"""
        return ()

    def _setup_stale(self, moved) -> None:
        """called in front of the raw setup that _enqueue_epochs() rebuilds; moved: per tensor of _resident() whether it was
        replaced, None in front of the first setup"""

    def _before_epochs(self) -> None:
        """called in front of issuing or capturing epochs, outside any capture: what the launches read is brought up to date"""

    def _step_weights(self, bw):
        """(weights argument, flags) of one of the epochs' planned launches; bw: the minibatch's RawBatch.weights"""
        return bw, self._flags

    def _graph_key_extra(self):
        """what captured epochs depend on beyond the parameter buffer, the run length and the schedule slot"""
        return None

    def _alpha_for(self, k: int) -> float:
        """the alpha of minibatch k of the epoch being issued (may keep it in self.alpha, as the reference's loop does)"""
        return self.alpha

    def _alpha_scheduled(self) -> bool:
        """does alpha change from step to step?  Then the device-side schedule carries a column of it (_sched_alphas)"""
        return False

    def _sched_alphas(self, j: np.ndarray) -> np.ndarray:
        """the schedule's alpha column under _alpha_scheduled(): row j[i] is minibatch j[i] % batch_num of epoch
        epoch_cnt + j[i] // batch_num"""
        raise NotImplementedError

    def _after_replay(self, n: int) -> None:
        """n epochs were replayed (epoch_cnt not yet moved on): host-side values that eagerly issued steps leave behind"""

    def _setup_ranges(self, model):
        """What one optimiser step exchanges and updates on this rank: `_ar_lo` = first float of the flat
        gradient that is all-reduced (through the loss tail), `_adam_ranges` = (offset, length) pieces of the
        flat buffers this rank applies Adam to."""
        st = self.state
        # tables indexed by user: InvPref keeps two (invariant, env-aware), PureMF one
        self._user_tables = (0,) if self._pure else (0, 2)
        if self.shard_mode == 'users':
            lo, hi = self.shard.user_range(model.user_num)
            D = model.factor_num
            self._ar_lo = st.offsets[1]                      # the item table that follows the user tables: start of the replicated part
            self._adam_ranges = [(st.offsets[i] + lo * D, (hi - lo) * D) for i in self._user_tables] + \
                                [(self._ar_lo, st.n - self._ar_lo)]
            self._adam_ranges = [r for r in self._adam_ranges if r[1] > 0]
        else:
            self._ar_lo = 0
            self._adam_ranges = [(0, st.n)]
            if self.exchange == 'scatter' and self.world_size > 1:
                chunk = st.cap // self.world_size          # whole 256-byte lines (FlatState.cap)
                lo = min(self.rank * chunk, st.n)
                self._adam_ranges = [(lo, min(chunk, st.n - lo))] if st.n > lo else []

    def _row_tables(self):
        """(user tables, item tables, (offset, length) of the flat buffers' tail that holds the small tensors): how the rows a
        minibatch touches are addressed (touched_row_offsets) -- the packed exchange and lazy Adam"""
        st = self.state
        n_tabs = len(st.shapes)
        user_tabs = self._user_tables
        item_tabs = tuple(i + 1 for i in user_tabs)                     # (state_dict order: every user table is followed by its item table)
        big = sorted(user_tabs + item_tabs)
        small = [i for i in range(n_tabs) if i not in big]
        if small and min(st.offsets[i] for i in small) < max(st.offsets[i] for i in big):
            raise ValueError('the small tables must follow the big ones in the flat buffers')
        tail_off = min((st.offsets[i] for i in small), default=st.n)
        return user_tabs, item_tabs, (int(tail_off), int(st.n - tail_off))

    def _setup_packed(self, users_all, items_all):
        """The packed exchange of a row-sharded run (INVPREF_EXCHANGE=packed): the minibatches are static (utils.mini_batch,
        utils.py:12-19), so the rows of the four big tables that the GLOBAL minibatch k touches -- on any rank -- are known
        up front.  Every other row's gradient is zero everywhere (the planned pass writes zeros there, the plan-free one
        leaves the zeroed buffer alone; the dense regulariser only reaches the classifier), so the step all-reduces
        [touched rows | small tables] through one packed buffer instead of the whole flat gradient.  Same sums, same Adam:
        results equal the "allreduce" exchange up to the order in which the collective adds the ranks' terms.
        Worth it when a global minibatch touches a small share of the rows (a strong-scaling split of one 8 192-row Yahoo
        minibatch: 2.7 x fewer bytes); a weak-scaling run at 8 ranks touches nearly every user row."""
        st, D = self.state, self.model.factor_num
        u = users_all.cpu().numpy().astype(np.int64)
        v = items_all.cpu().numpy().astype(np.int64)
        user_tabs, item_tabs, self._packed_tail = self._row_tables()
        big = user_tabs + item_tabs
        self._packed_rows, most = [], 0
        for k in range(self.batch_num):
            lo, hi = k * self.batch_size, min((k + 1) * self.batch_size, self.n_total)
            offs = touched_row_offsets(u[lo:hi], v[lo:hi], st.offsets, user_tabs, item_tabs, D)
            self._packed_rows.append(torch.from_numpy(offs).to(self.device))
            most = max(most, len(offs))
        self._packed_vec = D % 4 == 0 and all(st.offsets[i] % 4 == 0 for i in big)
        self._packed_buf = torch.zeros(most * D + self._packed_tail[1] + 4, dtype=torch.float32, device=self.device)
        self.packed_floats = [int(r.numel()) * D + self._packed_tail[1] for r in self._packed_rows]   # on the wire, per minibatch

    def _exchange_gradient(self, k: Optional[int] = None):
        """the step's exchange in front of Adam (also on the 1-rank group of the forced sharded path: the same
        collectives, captured and replayed like on N ranks); k: the minibatch (the packed exchange's row list)"""
        st = self.state
        if self.exchange == 'scatter':
            reduce_scatter_sum_(st.grad_full[:st.cap], self.rank, self.world_size, self.process_group)
        elif self.exchange == 'packed' and k is not None:
            rows, (t_off, t_len) = self._packed_rows[k], self._packed_tail
            buf = self._packed_buf[:self.packed_floats[k]]
            D = self.model.factor_num
            ops.pack_rows(st.grad, rows, D, t_off, t_len, buf, self._packed_vec)
            all_reduce_sum_(buf, self.process_group)
            ops.unpack_rows(st.grad, rows, D, t_off, t_len, buf, self._packed_vec)
        else:
            all_reduce_sum_(st.grad[self._ar_lo:], self.process_group)

    def _exchange_parameters(self):
        """the step's exchange behind Adam (scatter mode: every rank updated its own slice of the flat buffer)"""
        if self.exchange == 'scatter':
            all_gather_chunks_(self.state.param_full, self.rank, self.world_size, self.process_group)

    def sync_parameters(self) -> None:
        """User-sharded runs: bring every rank's copy of the user tables up to date (each rank contributes its
        own rows; one all-reduce per table).  Called before evaluations and at the end of train(); a no-op
        otherwise.  The Adam moments of foreign rows are not exchanged (nothing reads them)."""
        if self.world_size == 1 or self.shard_mode != 'users':
            return
        lo, hi = self.shard.user_range(self.model.user_num)
        for i in self._user_tables:
            view = self.state.p_views[i]
            tmp = torch.zeros_like(view)
            tmp[lo:hi] = view[lo:hi]
            all_reduce_sum_(tmp, self.process_group)
            view.copy_(tmp)

    def _before_evaluation(self) -> None:
        self.sync_parameters()

    def _after_training(self) -> None:
        self.sync_parameters()  # (user-sharded runs: every rank ends with the complete model)
        self._check_alt_error()

    def _all_reduce_step(self):
        """the one exchange of an optimiser step: the shared part of the flat gradient + the loss tail"""
        all_reduce_sum_(self.state.grad_ext[self._ar_lo:], self.process_group)

    # ------------------------------------------------------------------ lazy Adam
    def set_lazy_adam(self, enabled: bool) -> None:
        """Opt in to (or out of) lazy Adam at an epoch boundary: an optimiser step updates the rows of the user and item tables
        whose ids occur in its minibatch, and every element of the small tensors, by the usual rule with the GLOBAL step
        counter; every other row keeps its parameters and moments bit for bit.  One step is the planned gradient pass over the
        touched rows followed by ONE torch.ops.invpref.adam_rows_ launch, so its cost follows the minibatch and not the tables
        (DESIGN.md §4.9).  A lazy step equals a dense step with the untouched rows put back; the trajectory therefore differs
        from torch.optim.Adam over dense embeddings -- the reference's -- whose untouched rows keep moving on their momentum.
        Off (the default) nothing changes: the same launches, the same bits.  Switching clears the captured epoch graphs."""
        enabled = bool(enabled)
        if enabled:
            why = self._lazy_adam_unsupported
            if why is None and (self.world_size > 1 or self._force_sharded_path):
                why = 'lazy Adam is single-process: a sharded step exchanges and updates whole ranges of the flat buffers'
            if why is not None:
                raise NotImplementedError(f'{type(self).__name__}.set_lazy_adam: {why}')
        if enabled == self._lazy:
            return
        if enabled:
            self._alt_parked = self._alt if self._alt is not None else self._alt_parked
            if self._grad_stale:
                # dense unfused steps leave their gradient behind; a lazy step starts from -- and leaves -- an all-zero buffer
                self.state.grad.zero_()
                self._grad_stale = False
        self._lazy = enabled
        self._graphs.clear()
        if enabled and self._lazy_consts is None:
            st, D = self.state, self.model.factor_num
            user_tabs, item_tabs, tail = self._row_tables()
            self._lazy_consts = dict(tail=([tail[0]], [tail[1]]) if tail[1] else ([], []), tabs=(user_tabs, item_tabs),
                                     vec=D % 4 == 0 and all(st.offsets[i] % 4 == 0 for i in user_tabs + item_tabs))
        if getattr(self, '_raw_ptrs', None) is not None:
            if enabled:
                self._lazy_setup()
            elif self._alt is None:
                self._alt = self._alt_parked     # (_alt_setup keeps its plans and workspace)
            self._alt_setup()

    def _lazy_setup(self):
        """What the static minibatches need under lazy Adam, built once and kept on the device: per minibatch the list of
        touched row offsets and the row plan WITHOUT streamed rows (the dense plans' device buffers, shared)."""
        if self._lazy_state is not None and self._lazy_state['plans_of'] is self._plans:
            return
        st, D = self.state, self.model.factor_num
        user_tabs, item_tabs = self._lazy_consts['tabs']
        u, v = self.users_tensor.cpu().numpy(), self.items_tensor.cpu().numpy()
        rows = [torch.from_numpy(touched_row_offsets(u[b.lo:b.lo + b.n], v[b.lo:b.lo + b.n], st.offsets, user_tabs, item_tabs,
                                                     D)).to(self.device) for b in self._raw_batches]
        self._lazy_state = dict(
            rows=rows, plans_of=self._plans,
            plans=None if self._plans is None else [planlib.without_streamed_rows(dp) for dp in self._plans])

    def _lazy_adam(self, rows: torch.Tensor, sched=None) -> None:
        """the launch that ends a lazy step: Adam on the listed rows and the small tensors, their gradient cleared"""
        st, L = self.state, self._lazy_consts
        ops.adam_rows_(st.param, st.grad, st.exp_avg, st.exp_avg_sq, rows, self.model.factor_num, L['tail'][0], L['tail'][1],
                       st.step, self.lr, zero_grad=True, vec_ok=L['vec'], sched=sched)

    def _lazy_batch_rows(self, users, items) -> torch.Tensor:
        """the touched row offsets of a caller-supplied minibatch (device tensors or host arrays of ids), on the device"""
        user_tabs, item_tabs = self._lazy_consts['tabs']
        dev = lambda x: (torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x.detach()).to(self.device)  # noqa: E731
        return touched_row_offsets(dev(users), dev(items), self.state.offsets, user_tabs, item_tabs, self.model.factor_num)

    # row plans of caller-supplied minibatches, keyed by the identity of the tensors they were built from: (data_ptr,
    # length, _version) of users / items / scores -- a slice of a resident tensor that nobody has written to keeps all three
    _BATCH_PLAN_CACHE_MAX = 4096
    _BATCH_PLAN_CACHE_MAX_FOREIGN = 128

    def _cached_batch_plan(self, users, items, scores):
        # (INVPREF_NO_BATCH_PLAN_CACHE=1, test hook: every caller-supplied minibatch plan-free, as an unseen one runs)
        if not (self.use_plan and self.world_size == 1 and not self._unfused and not self._force_sharded_path
                and users.is_cuda and users.numel() > 0 and users.is_contiguous() and items.is_contiguous()
                and os.environ.get('INVPREF_NO_BATCH_PLAN_CACHE', '0') != '1'):
            return None
        key = tuple(x for t in (users, items, scores) for x in (t.data_ptr(), t.numel(), t._version, t.dtype))
        # The identity of a tensor (address, length, version counter) names its CONTENT only while the memory is the
        # manager's own: a slice of the resident interaction arrays (what the reference's loop hands over, train.py:204-233)
        # cannot be freed and reallocated behind the manager's back.  Any other tensor -- a freshly allocated batch comes
        # back from the caching allocator at the same address with version 0 -- is keyed by an order-sensitive checksum of its
        # ids and scores as well (three small kernels and a read-back per step), is planned at its SECOND sighting only,
        # and shares a small cache.
        resident = all(any(t.untyped_storage().data_ptr() == r.untyped_storage().data_ptr()
                           for r in (self.users_tensor, self.items_tensor, self.scores_tensor)) for t in (users, items, scores))
        if not resident:
            n = users.numel()
            pos = getattr(self, '_batch_pos', None)
            if pos is None or pos.numel() < n:
                pos = self._batch_pos = torch.arange(max(n, 1 << 16), dtype=torch.int64, device=users.device) * 2654435761 + 1
            # (a multiplicative mix of the three words per interaction, xor-folded: not linear in (u, i) as u * a + i * b was)
            mix = (users.to(torch.int64) * -7046029254386353131) ^ (items.to(torch.int64) * -4417276706812531889 + 0x2545F491) ^ \
                (scores.float().contiguous().view(torch.int32).to(torch.int64) * 40503)
            mix = mix ^ (mix >> 29)
            # (the content IS the key: addresses and version counters of foreign tensors say nothing)
            key = ('foreign', n, users.dtype, items.dtype, int((mix * pos[:n]).sum().item()))
        # (foreign minibatches have a small cache of their own -- filling it never evicts the resident slices' plans -- and a
        #  hit is trusted only after the ids and labels kept with the plan compare equal: the checksum is a filter, not an
        #  identity -- ADVICE r05)
        cache = self._batch_plans if resident else self._batch_plans_foreign
        hit = cache.get(key)
        if hit is not None and not resident and hit != 1:
            hit, ku, ki, ky = hit
            if not (torch.equal(ku, users) and torch.equal(ki, items) and torch.equal(ky, scores.float())):
                hit = 1                         # a checksum collision: plan this content afresh, replacing the entry
        if hit is None:
            if len(cache) >= (self._BATCH_PLAN_CACHE_MAX if resident else self._BATCH_PLAN_CACHE_MAX_FOREIGN):
                cache.clear()
            # first sighting: with the native builder a plan costs about a millisecond (and the ids' trip to the host), so it
            # is made at once -- INVPREF_BATCH_PLAN_AT=2 waits for the second sighting (a caller that never repeats a
            # minibatch pays nothing for plans it would not reuse) and runs the first one plan-free
            if os.environ.get('INVPREF_BATCH_PLAN_AT', '1') != '1' or planlib._native_lib() is None or not resident:
                cache[key] = 1
                return None
            hit = 1
        if hit == 1:                            # invert the scatter pattern once (host side)
            hit = self._batch_plan(users.cpu().numpy(), items.cpu().numpy(), scores.float().cpu().numpy())
            cache[key] = hit if resident else (hit, users.clone(), items.clone(), scores.float().clone())
        return hit

    def _batch_plan(self, users: np.ndarray, items: np.ndarray, scores: np.ndarray):
        """the row plan of ONE caller-supplied minibatch (host arrays), built and uploaded"""
        return planlib.upload(planlib.build_row_plan(users, items, scores, self.model.user_num, self.model.item_num,
                                                     factor_num=self.model.factor_num,
                                                     env_num=self._env_count), self.device)

    # ---- the epoch loop: every per-minibatch argument (views of the resident interaction arrays, the row plan,
    #      the zero-initialised scratch) is prepared once; a step is one or two torch.ops.invpref.* calls
    #      (+ the collective in a sharded run) and nothing is read back
    def _raw_setup(self):
        st = self.state
        L = _capi.lib()
        # one graph replays up to _graph_epochs epochs (fewer, longer launches: the GPU idles ~60 us
        # between two replays); each epoch of a replay writes its own [batch_num, 6] slice of the loss buffer
        self._graph_epochs = max(1, min(8, 2048 // self.batch_num))
        self._epoch_losses = torch.zeros(self._graph_epochs, self.batch_num, 6, dtype=torch.float32, device=self.device)
        self._loss_slot = 0
        self._raw_ptrs = tuple(t.data_ptr() for t in self._resident())     # (not None: the setup exists)
        self._raw_batches = []
        for k in range(self.batch_num):
            lo, hi = self.shard.local_batch_bounds(k)
            self._raw_batches.append(RawBatch(lo, hi - lo, self.shard.global_batch_len(k), self.users_tensor[lo:hi],
                                              self.items_tensor[lo:hi], self.scores_tensor[lo:hi], *self._batch_inputs(lo, hi)))
        if not hasattr(self, '_adam_ranges'):
            self._adam_ranges = [(0, st.n)]
        rg = self._adam_ranges
        self._adam_ranges_ok = len(rg) <= 4 and all(o % 4 == 0 and n % 4 == 0 for o, n in rg)   # one ranged launch can do it
        self._adam_ranges_one = len(rg) > 1 and self._adam_ranges_ok
        if self.use_plan and self._plans is None:
            t0 = time.perf_counter()
            u, v = self.users_tensor.cpu().numpy(), self.items_tensor.cpu().numpy()
            y = self.scores_tensor.cpu().numpy()
            # every minibatch's plan in one call: parameters resolved per minibatch, the arrays built natively on a thread
            # pool (csrc/invpref_plan.cpp; plan.py's numpy builder, native=False, is the reference implementation)
            last = self._raw_batches[-1]
            offs = np.array([b.lo for b in self._raw_batches] + [last.lo + last.n], np.int64)
            contiguous = all(offs[k] + b.n == offs[k + 1] for k, b in enumerate(self._raw_batches))
            kw = dict(factor_num=self.model.factor_num, user_range=self.shard.user_range(self.model.user_num),
                      env_num=self._env_count)
            if contiguous:
                pls = planlib.build_row_plans(u, v, y, offs, self.model.user_num, self.model.item_num, **kw)
            else:
                pls = [planlib.build_row_plan(u[b.lo:b.lo + b.n], v[b.lo:b.lo + b.n], y[b.lo:b.lo + b.n], self.model.user_num,
                                              self.model.item_num, **kw) for b in self._raw_batches]
            self._plans = [planlib.upload(pl, self.device) for pl in pls]
            self.plan_build_s = time.perf_counter() - t0     # host-side, once per run (reported by bench.py)
        if self._lazy:
            self._lazy_setup()
        self._alt_setup()
        if self.use_plan and self.users_tensor.is_cuda:
            # every plan shares ONE scratch (records + partial slabs; nothing carries over between steps): size it for
            # the largest BEFORE any graph capture bakes its address in
            t = self._make_tables(st.p_views)
            self.workspace.get_zeroed(max(L.invpref_rows_workspace_bytes(C.byref(t), C.byref(dp.struct))
                                          for dp in self._plans))

    # ---- the alternating form: ONE launch per optimiser step (include/invpref_hip.h: invpref_mstep_alt_hip; csrc/step_alt.hpp).
    # Inside a run of whole epochs launch i evaluates minibatch i % batch_num from the users' side (even i) or the items'
    # (odd i): the side applies the previous step's pending update to its rows, evaluates, applies its own update and
    # pushes contribution rows for the other side; a flush launch ends the run.  Nothing outside a run ever sees the
    # intermediate state; parameters and moments are updated in place (no buffer swap).
    def _alt_setup(self):
        st = self.state
        prev, self._alt = self._alt, None
        # (INVPREF_ALT=0, test hook: the two-launch form, which every other shape takes, at the alternating form's shapes)
        if not (self.use_plan and self._plans and self.users_tensor.is_cuda and self._fused_seq()
                and os.environ.get('INVPREF_ALT', '1') == '1' and ops.alt_supported(st.p_views)):
            return
        n_cap = max(b.n for b in self._raw_batches)
        host = getattr(self, '_alt_host', None)
        if host is None:
            host = self._alt_host = (self.users_tensor.cpu().numpy(), self.items_tensor.cpu().numpy(),
                                     self.scores_tensor.cpu().numpy().astype(np.float32))
        # The alternating form EVALUATES from the items' side every other step: a row's interactions are spread over at most 32
        # slices and each slice evaluates its share one after the other (~1.3 us each).  With 8 192-row Yahoo minibatches the
        # hottest item has 60-77 interactions -- three per slice; with one minibatch per epoch (SURVEY 8(d)-4's B = N variant:
        # 250 interactions per item on average) the chains are tens of evaluations long and the two-launch form, whose item
        # side only SUMS contribution rows, is twice as fast (measured: 199 vs 101 us per step).  Decided on the first
        # minibatch's heaviest row; INVPREF_ALT_MAX_CHAIN overrides the bound (test hook: either form at one shape).
        lo0, n0 = self._raw_batches[0].lo, self._raw_batches[0].n
        heavy = max(int(np.bincount(host[0][lo0:lo0 + n0]).max(initial=0)), int(np.bincount(host[1][lo0:lo0 + n0]).max(initial=0)))
        if -(-heavy // 32) > int(os.environ.get('INVPREF_ALT_MAX_CHAIN', '6')):
            return
        self._alt = dict(plans={}, host_plans={}, n_cap=n_cap, partials_cap=n_cap // 4 + n_cap // 8 + 128, ws=None,
                         build_s=0.0)
        if prev is not None and prev['n_cap'] == n_cap:
            # (the plans depend on the ids and the minibatch bounds only -- not on the environment / weight arrays whose
            #  re-homing brought us here: keep them, their slot choice and the workspace)
            self._alt.update({k: prev[k] for k in ('plans', 'ws', 'slots') if k in prev})

    def _alt_keys(self, n: int, steps: Optional[int] = None):
        """(k_prev, k, side) of every launch of a run of n epochs (or of its first `steps` minibatches), the flush (k = None) last"""
        bn = self.batch_num
        total = n * bn if steps is None else steps
        keys = [(None, 0, 0)] + [((i - 1) % bn, i % bn, i & 1) for i in range(1, min(total, 2 * bn + 1))]
        return keys + [((total - 1) % bn, None, total & 1)]     # (the plan sequence is periodic after the first launch)

    def _alt_prepare(self, n: int, steps: Optional[int] = None):
        """builds (natively, one call: csrc/invpref_plan.cpp) and uploads every plan a run of n epochs (or of its first `steps`
        minibatches) needs, and the run's workspace -- BEFORE a graph capture starts: host-to-device copies and allocations
        are not capturable"""
        A = self._alt
        need = [key for key in dict.fromkeys(self._alt_keys(n, steps)) if key not in A['plans']]
        if need:
            t0 = time.perf_counter()
            u, v, y = self._alt_host
            rng = lambda k: None if k is None else (self._raw_batches[k].lo, self._raw_batches[k].n)   # noqa: E731
            if 'slots' not in A:   # group slots per round of either side's launches, from the first minibatch
                lo, n0 = self._raw_batches[0].lo, self._raw_batches[0].n
                A['slots'] = (planlib.alt_slots_for(u[lo:lo + n0], self.model.user_num, planlib.ALT_PER_SLICE),
                              planlib.alt_slots_for(v[lo:lo + n0], self.model.item_num, planlib.ALT_PER_SLICE))
            hps = planlib.build_alt_plans(u, v, y, [(rng(k), rng(kp), side) for kp, k, side in need], self.model.user_num,
                                          self.model.item_num, factor_num=self.model.factor_num, slots_u=A['slots'][0],
                                          slots_i=A['slots'][1])
            for key, hp in zip(need, hps):
                if hp['n_tasks'] > A['partials_cap']:
                    raise _capi.InvPrefError('alt plan: more job tasks than the workspace was sized for')
                A['plans'][key] = planlib.upload_alt(hp, self.device)
            A['build_s'] += time.perf_counter() - t0
        if A['ws'] is None:
            A['ws'] = ops.AltWorkspace(self.state.p_views, A['n_cap'], A['partials_cap'], pure=self._pure)

    def _alt_plan(self, k_prev, k, side: int, partials_prev: int):
        """device plan of the launch that evaluates minibatch k (None: a flush) from `side` after a launch that evaluated
        minibatch k_prev (None: first launch of a run) and left `partials_prev` partial slabs"""
        return planlib.alt_with_partials(self._alt['plans'][(k_prev, k, side)], partials_prev)

    def _issue_epochs_alt(self, sched: bool, n: int, steps: Optional[int] = None):
        """n epochs of alternating launches + the flush; `steps`: only the first `steps` minibatches of the run"""
        st, A, bn = self.state, self._alt, self.batch_num
        total = n * bn if steps is None else steps
        if not torch.cuda.is_current_stream_capturing():
            self._alt_prepare(n, steps)
        k_prev, tasks_prev, alpha = None, 0, self.alpha
        for i in range(total):
            j, k = divmod(i, bn)
            self._loss_slot = j
            dp = self._alt_plan(k_prev, k, i & 1, tasks_prev)
            b = self._raw_batches[k]
            alpha = self._alpha_for(k)
            st.step += 1
            sc = (self._sched['state'], self._sched['table'], st.step & 1) if sched else None
            lp = self._epoch_losses[(i - 1) // bn, (i - 1) % bn] if i else None
            wts, flags = self._step_weights(b.weights)
            ops.mstep_alt(st.p_views, st.m_views, st.v_views, dp, b.env_ids, wts, b.global_n,
                          self._raw_batches[k_prev].global_n if k_prev is not None else b.global_n, self._coefs(alpha), flags, lp,
                          st.step, self.lr, A['ws'], i & 1, pure=self._pure, sched=sc)
            k_prev, tasks_prev = k, dp.n_tasks
        # the flush: the other side's rows take the last step's update, the last fold (in the LAST step's schedule slot)
        dp = self._alt_plan(k_prev, None, total & 1, tasks_prev)
        sc = (self._sched['state'], self._sched['table'], st.step & 1) if sched else None
        bnorm = self._raw_batches[k_prev].global_n
        ops.mstep_alt(st.p_views, st.m_views, st.v_views, dp, None, None, bnorm, bnorm, self._coefs(alpha), self._flags,
                      self._epoch_losses[(total - 1) // bn, (total - 1) % bn], st.step, self.lr, A['ws'], total & 1,
                      pure=self._pure, sched=sc)
        self._loss_slot = 0

    def alt_error(self) -> int:
        """1 if a workgroup of an alternating launch ever gave up waiting for its step's small tables (host sync; never in a
        healthy run).  Sticky on the device until _check_alt_error() has raised for it."""
        A = getattr(self, '_alt', None)
        return 0 if not A or A['ws'] is None else A['ws'].error()

    def _check_alt_error(self) -> None:
        """Called wherever the host reads results of a run back anyway (train_epochs(sync=True), loss_dicts of a deferred
        run, the end of train()): a job workgroup that timed out staged NaN tables, so the run's numbers are void --
        say so loudly instead of handing them back (csrc/step_alt.hpp: alt_stage_finish)."""
        if self.alt_error():
            self._alt['ws'].reset_error()
            raise _capi.InvPrefError(
                'alternating M-step: a job workgroup gave up waiting for the fold blocks of its launch (ALT_POLL_MAX polls); '
                'the parameters of this run are invalid (NaN small tables were staged).  Re-create the manager; '
                'INVPREF_ALT=0 selects the two-launch form, which has no in-launch dependency.')

    def _raw_step(self, k: int, alpha: float, stream=None, mid_event=None, sched=False):
        st = self.state
        if not sched:
            self._sched_synced = False
        b = self._raw_batches[k]
        coefs = self._coefs(alpha)
        lazy = self._lazy
        multi = self.world_size > 1 or self._force_sharded_path or self._unfused or lazy
        # every step's six loss terms go straight into the epoch's loss buffer (this rank's partial sums in a
        # sharded run: they are all-reduced once per epoch, not per step)
        lp = self._epoch_losses[self._loss_slot, k]
        if self.use_plan and not multi:
            # fused M-step + Adam: one pass, gradient never stored, parameters ping-pong
            st.step += 1
            sc = (self._sched['state'], self._sched['table'], st.step & 1) if sched else None
            wts, flags = self._step_weights(b.weights)
            ops.mstep_rows_adam(st.p_views, st.p_views_alt, st.m_views, st.v_views, self._plans[k], b.env_ids, b.scores, wts,
                                b.global_n, coefs, flags, lp, st.step, self.lr, self.workspace, pure=self._pure, sched=sc,
                                mid_event=mid_event)   # (profiling: recorded between the step's two launches)
            st.swap()
            return
        st.step += 1
        # graph capture: per-step scalars (Adam bias corrections, a scheduled alpha) come from the device-side
        # schedule, read by the gradient pass and moved on by the ranged Adam launch that ends the step
        sc = (self._sched['state'], self._sched['table'], st.step & 1) if sched else None
        if self.use_plan:
            wts, flags = self._step_weights(b.weights)
            # (lazy Adam: the plan without streamed rows -- the pass writes the touched rows and the small tensors only)
            plan = self._lazy_state['plans'][k] if lazy else self._plans[k]
            self._gradient_pass(k, plan, b.users, b.items, b.env_ids, b.scores, wts, b.global_n, coefs, flags, lp, sc)
        else:
            self._gradient_pass(k, None, b.users, b.items, b.env_ids, b.scores, b.weights, b.global_n, coefs, self._flags, lp, None)
        if multi and not lazy:
            if self.world_size > 1 or self._collective_ok:
                self._exchange_gradient(k)   # all-reduce (whole or packed), or reduce-scatter (this rank keeps its slice of the sum)
        self._after_gradient_pass(k, lp)
        if mid_event is not None:
            mid_event.record()
        if lazy:
            # the buffer was all-zero before the pass and this launch clears exactly what the pass (and the hook) wrote: it is
            # all-zero again, so _grad_stale never asks for a whole-buffer zero_()
            self._lazy_adam(self._lazy_state['rows'][k], sched=sc)
            return
        # the planned gradient pass overwrites every row it is responsible for, so the gradient buffer needs no zeroing
        zero = not self.use_plan
        if self.use_plan:
            self._grad_stale = True   # see _step()
        if self._adam_ranges_one or sched:   # every piece in one launch
            ops.adam_ranges_(st.param, st.grad, st.exp_avg, st.exp_avg_sq, [o for o, _ in self._adam_ranges],
                             [ln for _, ln in self._adam_ranges], st.step, self.lr, zero_grad=zero, sched=sc)
        else:
            for o, ln in self._adam_ranges:
                ops.adam_(st.param[o:o + ln], st.grad[o:o + ln], st.exp_avg[o:o + ln], st.exp_avg_sq[o:o + ln], st.step,
                          self.lr, zero_grad=zero)
        if multi and (self.world_size > 1 or self._collective_ok):
            if zero and self.exchange == 'scatter' and self.world_size > 1:
                st.grad.zero_()   # plan-free gradients ADD: the slices this rank's Adam did not clear must start from zero too
            self._exchange_parameters()

    def _gradient_pass(self, k, plan, users, items, env_ids, scores, weights, batch_norm: int, coefs, flags: int,
                       losses6: torch.Tensor, sched=None) -> None:
        """The gradient pass of the unfused sequence: the gradient of one minibatch into state.g_views, its loss terms into
        losses6.  k: the static minibatch, None for a caller-supplied one (baseline.py: _batch_step).  plan: its row plan
        (the planned pass OVERWRITES every row), None: the plan-free pass over users / items, which ADDS.  A manager whose
        loss is not the step's own overrides this (baseline.py: MACRTrainManager)."""
        st = self.state
        if plan is not None:
            ops.mstep_rows_grad(st.p_views, st.g_views, plan, env_ids, scores, weights, batch_norm, coefs, flags, losses6,
                                self.workspace, sched=sched)
        else:
            ops.mstep_grad(st.p_views, st.g_views, users, items, env_ids, scores, weights, batch_norm, coefs, flags, losses6,
                           self.workspace)

    def _after_gradient_pass(self, k: int, losses6: torch.Tensor) -> None:
        """Hook of the unfused sequence (gradient pass -> [exchange] -> HERE -> Adam), minibatch k of epoch slot
        self._loss_slot: a manager whose loss has a term the step does not know adds its gradient into state.g_views and its
        value into losses6 (baseline.py: _DrawnTermMixin, the base of the WMF and CVIB managers).  Nothing is launched here."""

    # ---- device-side Adam schedule for graph replay (include/invpref_hip.h: InvPrefAdamSchedule)
    _SCHED_N = 8192

    def _sched_prepare(self, steps_ahead: int):
        """Device-side schedule for graph replay (InvPrefAdamSchedule): one row per optimiser step with the Adam
        scalars and, under the alpha schedule of train.py:214-217, that step's alpha.  Called at an epoch
        boundary: row j belongs to minibatch j % batch_num of epoch epoch_cnt + j // batch_num.
        A run of `steps_ahead` steps must fit into ONE table: the launch of a table's last step leaves its successor's
        scalars as they are (the kernels' `idx < sched_n` guard), so a longer run would go on with stale ones."""
        if steps_ahead > self._SCHED_N:
            raise _capi.InvPrefError(f'a replayed run of {steps_ahead} optimiser steps does not fit into the device-side '
                                     f'Adam schedule of {self._SCHED_N} rows (graphs_enabled() / _graph_epochs bound it)')
        st = self.state
        if self._sched is None:
            table = torch.zeros(self._SCHED_N, 8, dtype=torch.float32, device=self.device)
            state = torch.zeros(32, dtype=torch.int32, device=self.device)
            self._sched = dict(table=table, state=state, base=-(10 ** 9), host=None,
                               struct=_capi.AdamSchedule(state.data_ptr(), table.data_ptr(), self._SCHED_N))
        sc = self._sched
        first = st.step + 1
        alphas = self._alpha_scheduled()
        stale_alpha = alphas and not self._sched_synced   # the step -> (epoch, minibatch) mapping moved
        if first < sc['base'] or first + steps_ahead > sc['base'] + self._SCHED_N or stale_alpha:
            host = np.zeros((self._SCHED_N, 8), np.float32)
            _capi.call('invpref_adam_schedule_fill', host.ctypes.data, first, self._SCHED_N, self.lr, 0.9, 0.999, 1e-8)
            if alphas:
                host[:, 6] = self._sched_alphas(np.arange(self._SCHED_N))
            sc['table'].copy_(torch.from_numpy(host))
            sc['base'], sc['host'] = first, host
            self._sched_synced = False
        if not self._sched_synced:  # the device counter follows the host's after eager steps / refills
            st32, o = np.zeros(32, np.int32), 16 * (first & 1)  # the slot of the step about to run
            st32[o:o + 2] = first, sc['base']
            st32[o + 2:o + 10] = sc['host'][first - sc['base']].view(np.int32)
            sc['state'].copy_(torch.from_numpy(st32))
            self._sched_synced = True

    def _issue_epochs(self, stream, sched: bool, n: int):
        self._epoch_losses[:n].zero_()
        st = self.state
        # (eagerly issued epochs run the same launches as captured ones: graph replay == eager launches, bit for bit)
        if getattr(self, '_alt', None) is not None:
            self._issue_epochs_alt(sched, n)
            return
        for j in range(n):
            self._loss_slot = j
            for k in range(self.batch_num):
                self._raw_step(k, self._alpha_for(k), stream, sched=sched)
        self._loss_slot = 0

    def train_a_epoch(self) -> dict:
        """train.py:204-233, without the per-batch host syncs (one read-back per epoch)."""
        return self.train_epochs(1)[0]

    def train_epochs(self, n: int, sync: bool = True):
        """n consecutive train_a_epoch() calls with ONE host read-back at the end: the epochs are
        enqueued back to back, so the GPU does not idle between them while the host fetches losses
        (train() uses this between two evaluate/cluster events).  Returns the n loss dicts in order;
        with sync=False nothing is read back and the device tensor [n, 6] (LOSS_KEYS order) is returned
        instead -- loss_dicts() turns it into the dicts later."""
        dev, left = [], int(n)
        while left > 0:
            dev.append(self._enqueue_epochs(left))
            left -= dev[-1].shape[0]
        out = torch.cat(dev) if dev else torch.zeros(0, 6, device=self.device)
        if sync:
            self._check_alt_error()
        return self.loss_dicts(out) if sync else out

    def _enqueue_epochs(self, want: int) -> torch.Tensor:
        """Issues up to `want` epochs on the current stream and returns their mean losses as a device
        tensor [n_issued, 6].  On one GPU with a fixed alpha, runs of whole epochs (batch_num fused steps
        each) are captured once per (parameter-buffer parity, run length) into a HIP graph and replayed:
        one launch per run instead of 2*batch_num per epoch."""
        self.model.train()
        old, now = getattr(self, '_raw_ptrs', None), tuple(t.data_ptr() for t in self._resident())
        if old != now:
            self._setup_stale(None if old is None else tuple(a != b for a, b in zip(old, now)))
            self._raw_setup()
            self._graphs.clear()
        st = self.state
        self._before_epochs()
        # the fused single-GPU step, and the gradient-pass -> [all-reduce] -> ranged-Adam sequence of sharded runs and
        # wide rows (RCCL collectives record into a HIP graph like kernels do), are replayed as whole-epoch graphs
        fused_seq = self._fused_seq()
        graph_ok = self.graphs_enabled()
        g = None
        if graph_ok and self._graph_warm:
            n = min(want, self._graph_epochs)
            steps = n * self.batch_num
            self._sched_prepare(steps)
            fresh = self._graph_key(n) not in self._graphs
            try:
                g = self._graph_for(n)
            except Exception as exc:   # e.g. a collective library that cannot record into a graph: stay eager
                import warnings
                warnings.warn(f'HIP-graph capture of the epoch failed ({exc!r}); continuing with eager launches')
                g = None
            if fresh and self.world_size > 1:
                # graph or eager changes the order and the sizes of the collectives that follow (one loss all-reduce per
                # replayed run against one per epoch): a capture that failed on ANY rank puts EVERY rank on eager launches
                ok = torch.tensor([0 if g is None else 1], dtype=torch.int32, device=self.device)
                all_reduce_min_(ok, self.process_group)
                if int(ok.item()) == 0:
                    g = None
                    self._graphs.pop(self._graph_key(n), None)
            if g is None:
                self.use_graph = False
                self._graphs_agreed = None
                self._loss_slot = 0
        if g is not None:
            g.replay()
            st.step += steps
            if steps % 2 and fused_seq and self._alt is None:   # (the alternating form updates in place)
                st.swap()
            if self.world_size > 1:
                all_reduce_sum_(self._epoch_losses[:n], self.process_group)   # per-rank loss partials -> totals
            self._after_replay(n)
        else:
            n = 1
            self._issue_epochs(None, False, 1)
            if self.world_size > 1:
                all_reduce_sum_(self._epoch_losses[:1], self.process_group)   # per-rank loss partials -> totals
            self._graph_warm = True
            self._sched_synced = False
        self.epoch_cnt += n
        return self._epoch_losses[:n].mean(dim=1)

    def _fused_seq(self) -> bool:
        """one fused M-step + Adam launch per step (single GPU, rows of at most 128 floats), parameters ping-pong"""
        return self.world_size == 1 and not self._unfused and not self._force_sharded_path and not self._lazy

    def graphs_enabled(self) -> bool:
        """Are whole epochs replayed as HIP graphs?  (after the first, eagerly issued, epoch)"""
        if getattr(self, '_raw_ptrs', None) is None:
            self._raw_setup()
        mine = bool(self.use_graph and self.use_plan and self.users_tensor.is_cuda
                    and self.batch_num <= self._SCHED_N // 2
                    and (self._fused_seq() or (self._adam_ranges_ok and self._graph_collectives())))
        if self.world_size == 1:
            return mine
        # The decision must be the SAME on every rank (it fixes the sequence of collectives), but its inputs are not:
        # _adam_ranges_ok depends on this rank's row range (user-sharded runs with factor_num % 4 != 0).  Agreed once
        # per manager state with an all-reduce(MIN); a failed capture resets it (see _enqueue_epochs).
        if getattr(self, '_graphs_agreed', None) is None or self._graphs_agreed[0] != mine:
            ok = torch.tensor([1 if mine else 0], dtype=torch.int32, device=self.device)
            all_reduce_min_(ok, self.process_group)
            self._graphs_agreed = (mine, bool(int(ok.item())))
        return self._graphs_agreed[1]

    def _graph_collectives(self) -> bool:
        """May the step's all-reduce be captured?  Yes on the RCCL backend (or when there is none to capture);
        INVPREF_NO_COLLECTIVE_GRAPH=1 keeps the sharded loop eager (bench.py names it where a capture fails)."""
        if os.environ.get('INVPREF_NO_COLLECTIVE_GRAPH', '0') == '1':
            return False
        if self.world_size == 1 and not self._collective_ok:
            return True
        import torch.distributed as dist
        return dist.get_backend(self.process_group) == 'nccl'

    def _graph_key(self, n: int):
        return (self.state.p_views[0].data_ptr(), n, self.state.step & 1, self._graph_key_extra())

    def _graph_for(self, n: int):
        """The HIP graph of n epochs starting from the current parameter buffer (captured on first use)."""
        st = self.state
        key = self._graph_key(n)
        g = self._graphs.get(key)
        if g is None:
            if self._alt is not None:
                self._alt_prepare(n)
            step0, views0 = st.step, st.p_views
            g = torch.cuda.CUDAGraph()
            try:
                # (thread-local capture mode: the RCCL watchdog thread of a process group may query events meanwhile)
                with _gc_paused(), torch.cuda.graph(g, capture_error_mode='thread_local'):
                    self._issue_epochs(None, True, n)
            finally:
                # capture records, it does not run: put the host-side bookkeeping back
                st.step = step0
                if st.p_views is not views0:
                    st.swap()
            self._graphs[key] = g
        return g

    def prepare_graphs(self, run_lengths) -> None:
        """Captures the epoch graphs for the given run lengths (epochs per replay) and both parameter
        buffers ahead of time, so that no capture happens inside a timed loop.  Needs one eager epoch
        before it (train_epochs(1)); nothing is executed and no state changes."""
        if not self._graph_warm or getattr(self, '_raw_ptrs', None) is None:
            raise RuntimeError('prepare_graphs(): run one epoch first (train_epochs(1))')
        self._sched_prepare(self.batch_num)
        self._before_epochs()
        for n in sorted({min(max(1, int(x)), self._graph_epochs) for x in run_lengths}):
            step0 = self.state.step
            for _ in range(2):  # a fused step swaps the buffers and flips the schedule slot: both move together
                self._graph_for(n)
                if self._fused_seq() and self._alt is None:   # (the alternating form: in place, only the slot parity moves)
                    self.state.swap()
                self.state.step += 1
            self.state.step = step0
