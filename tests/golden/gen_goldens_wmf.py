#!/usr/bin/env python3
"""Generate the g19 WMF goldens under tests/golden/ by RUNNING THE REFERENCE.

Runs only in the build container (needs the reference checkout, CPU torch, one thread).  Like gen_goldens_expomf.py it imports
the reference's own ``baseline_models.py`` / ``baseline_train.py`` (never copied) and stores inputs + outputs as small ``.npz``
files (tests/golden/README_g19.md):

  g19_wmf_block     PureMatrixFactorization.forward(users, items, zeros) on the Cartesian list of seeded 37 x 53 blocks at
                    D = 24, 40, 64, 256 and the gradients autograd gives for both tables, once with ordinary scores and once
                    with three user rows whose scores are +-30 / +-100 (fp32 sigmoid exactly 1 / exactly 0)
  g19_wmf_<case>    WMFTrainManager trajectories on the g7 implicit data (tests/wmf_fixture.py CASES): the seed, every step's
                    selection, the per-epoch loss dicts, the tables after the first step and at the end, train_a_batch on
                    caller pairs with its selection, and the reference's distance from the fixture's float64 statement

The reference builds its imputation targets with torch.Tensor(n) -- uninitialised memory.  The generator zeroes that tensor
on the reference's manager before training (data handed to the reference, not a change of its code) and asserts afterwards
that it is still all zero.

Usage:  python tests/golden/gen_goldens_wmf.py [REFERENCE_ROOT]   (default: $INVPREF_REFERENCE_ROOT, else a `reference`
checkout next to the repository)
"""
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('INVPREF_REFERENCE_ROOT',
                                                           os.path.join(os.path.dirname(REPO), 'reference'))
sys.dont_write_bytecode = True
sys.modules.setdefault('seaborn', types.ModuleType('seaborn'))  # utils.py imports it, unused
sys.path.insert(0, REF)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import baseline_models as ref_models  # noqa: E402  (reference)
import baseline_train as ref_bt  # noqa: E402  (reference)

from wmf_fixture import (BLOCK_DIMS, CASES, EVAL_BATCH, block_case, caller_pairs, impute64, step64, trajectory64,  # noqa: E402
                         wmf_inputs)

CPU = torch.device('cpu')
KEYS = ['score_loss', 'L2_reg', 'L1_reg', 'loss']


class StubEvaluator:
    batch_size = EVAL_BATCH

    def evaluate(self):
        return {'stub': 0.0}


def load(model, tabs):
    model.load_state_dict({k: torch.from_numpy(v) for k, v in tabs.items()})


def gen_block():
    out = {}
    for D in BLOCK_DIMS:
        for sat in (False, True):
            Pu, Qi, Su, Si = block_case(D, sat)
            m = ref_models.PureMatrixFactorization(Pu.shape[0], Qi.shape[0], D)
            load(m, {'user_emb.weight': Pu, 'item_emb.weight': Qi})
            pairs = torch.cartesian_prod(torch.from_numpy(Su), torch.from_numpy(Si))
            loss = m(pairs[:, 0], pairs[:, 1], torch.zeros(len(pairs)))
            loss.backward()
            s = m(pairs[:, 0], pairs[:, 1]).detach().numpy().reshape(len(Su), len(Si))
            tag = f'd{D}_{"sat" if sat else "plain"}'
            out[tag + '_loss'] = np.array(float(loss))
            out[tag + '_gP'] = m.user_emb.weight.grad.numpy().copy()
            out[tag + '_gQ'] = m.item_emb.weight.grad.numpy().copy()
            out[tag + '_s'] = s.astype(np.float32)
            term, dP, dQ = impute64(Pu, Qi, Su, Si)
            x = Pu[Su].astype(np.float64) @ Qi[Si].astype(np.float64).T
            if sat:
                assert not np.any((np.abs(x) > 10) & (np.abs(x) < 25)), 'a score near the rounding of the sigmoid to 1'
                assert np.all(s[2] * (1 - s[2]) == 0) and (s[2] == 1).sum() > 0 and (s[2] == 0).sum() > 0
                ok = np.abs(x) < 10       # float64 has no clamp to speak of: compare the ordinary pairs' rows only
                rows = np.ones(len(Su), bool)
                rows[:3] = False
                e = np.abs(out[tag + '_gP'][Su[rows]] - dP[Su[rows]]).max()
                print(f'block D={D} saturated: ones {(s == 1).sum()} zeros {(s == 0).sum()} of {s.size}, loss {float(loss):.6f}, '
                      f'ordinary rows dP: reference vs float64 max abs {e:.2e} ({ok.sum()} ordinary pairs)')
            else:
                assert np.abs(x).max() < 6
                print(f'block D={D}: loss reference {float(loss):.8f} float64 {term:.8f} rel {abs(float(loss) - term) / term:.2e}, '
                      f'dP max abs {np.abs(out[tag + "_gP"] - dP).max():.2e} of {np.abs(dP).max():.2e}, '
                      f'dQ {np.abs(out[tag + "_gQ"] - dQ).max():.2e} of {np.abs(dQ).max():.2e}')
    np.savez_compressed(os.path.join(HERE, 'g19_wmf_block.npz'), **out)
    print('g19_wmf_block:', len(out), 'arrays')


def gen_case(name):
    (U, I, D, n, bs, epochs), data, init, cfg, kw, seed = wmf_inputs(name)
    model = ref_models.PureMatrixFactorization(U, I, D)
    load(model, init)
    mgr = ref_bt.WMFTrainManager(model=model, evaluator=StubEvaluator(), device=CPU, training_data=torch.from_numpy(data),
                                 batch_size=bs, epochs=epochs, evaluate_interval=10 ** 9, lr=cfg['lr'], L2_coe=cfg['L2_coe'],
                                 L1_coe=cfg['L1_coe'], **kw)
    mgr.zero_tensor.zero_()      # torch.Tensor(n) is uninitialised memory: the target the method means is 0
    ubs, ibs = kw['user_batch_size'], kw['item_batch_size']
    if name == 'd30_ragged':
        cnt = [(len(np.unique(data[lo:lo + bs, 0])), len(np.unique(data[lo:lo + bs, 1]))) for lo in range(0, n, bs)]
        assert all(cu > ubs and ci > ibs for cu, ci in cnt[:-1]) and cnt[-1][0] < ubs and cnt[-1][1] < ibs, cnt
        print('g19', name, 'distinct per minibatch: full ones at least', min(c[0] for c in cnt[:-1]), '/',
              min(c[1] for c in cnt[:-1]), 'last', cnt[-1])

    # ---- observe: the permutations numpy hands out, and the pair list the model sees
    perms, sels, state = [], [], {'calls': 0, 'batch': None, 'first': None}
    orig_shuffle, orig_forward = np.random.shuffle, model.forward

    def shuffle(a):
        orig_shuffle(a)
        perms.append(a.copy())

    def forward(users_id, items_id, ground_truth=None):
        if ground_truth is not None:
            if state['calls'] % 2 == 0:
                state['batch'] = (users_id.numpy().copy(), items_id.numpy().copy())
            else:
                ru, ri = perms[-2], perms[-1]
                uu, ui = np.unique(state['batch'][0]), np.unique(state['batch'][1])
                Su, Si = uu[ru[:ubs]], ui[ri[:ibs]]
                want = torch.cartesian_prod(torch.from_numpy(Su), torch.from_numpy(Si))
                assert torch.equal(users_id, want[:, 0]) and torch.equal(items_id, want[:, 1])
                assert torch.equal(ground_truth, torch.zeros(len(want)))
                sels.append((Su, Si))
            state['calls'] += 1
        return orig_forward(users_id, items_id, ground_truth)

    np.random.shuffle, model.forward = shuffle, forward
    try:
        np.random.seed(seed)
        # the first step alone, for the tables after it; then the run proper from the same seed and tables
        first = next(iter(ref_bt.mini_batch(bs, mgr.users_tensor, mgr.items_tensor, mgr.scores_tensor)))
        mgr.train_a_batch(*first)
        first_tabs = {k: p.numpy().copy() for k, p in model.state_dict().items()}
        sel_first = sels.pop()
        load(model, init)
        mgr.optimizer = torch.optim.Adam(model.parameters(), lr=cfg['lr'])
        np.random.seed(seed)
        (losses, loss_epochs), _ = mgr.train(silent=True)
        assert len(sels) == epochs * mgr.batch_num and all(np.array_equal(a, b) for a, b in zip(sel_first, sels[0]))
        final = {k: p.numpy().copy() for k, p in model.state_dict().items()}
        pairs = caller_pairs(U, I, data)
        d = mgr.train_a_batch(*(torch.from_numpy(pairs[:, j]) for j in (0, 1)), torch.from_numpy(pairs[:, 2]).float())
        batch_sel = sels.pop()
        batch_tabs = {k: p.numpy().copy() for k, p in model.state_dict().items()}
    finally:
        np.random.shuffle = orig_shuffle
    assert bool((mgr.zero_tensor == 0).all()), 'zero_tensor must still be all zero'

    # ---- the same draws from the seeded stream alone, in the reference's order
    np.random.seed(seed)
    for s, (Su, Si) in enumerate(sels + [batch_sel]):
        b = s % mgr.batch_num
        rows = data[b * bs:(b + 1) * bs] if s < len(sels) else pairs
        uu, ui = np.unique(rows[:, 0]), np.unique(rows[:, 1])
        ru, ri = np.arange(len(uu)), np.arange(len(ui))
        np.random.shuffle(ru)
        np.random.shuffle(ri)
        assert np.array_equal(Su, uu[ru[:ubs]]) and np.array_equal(Si, ui[ri[:ibs]]), s

    traj = np.array([[d_[k] for k in KEYS] for d_ in losses], np.float64)
    t64, first64, (P64, Q64), opt = trajectory64(name, sels)
    dist_loss = float(np.max(np.abs(traj - t64) / np.abs(t64)))
    dist_tab = float(max(np.abs(final['user_emb.weight'] - P64).max(), np.abs(final['item_emb.weight'] - Q64).max()))
    dist_first = float(max(np.abs(first_tabs['user_emb.weight'] - first64[0]).max(),
                           np.abs(first_tabs['item_emb.weight'] - first64[1]).max()))
    terms, gP, gQ = step64(P64, Q64, pairs[:, 0], pairs[:, 1], pairs[:, 2].astype(np.float64), batch_sel[0], batch_sel[1],
                           cfg['L2_coe'], cfg['L1_coe'], kw['imputation_coe'])
    opt.step((P64, Q64), (gP, gQ))
    batch_loss = np.array([d[k] for k in KEYS])
    dist_batch_loss = float(np.max(np.abs(batch_loss - terms) / np.abs(terms)))
    dist_batch_tab = float(max(np.abs(batch_tabs['user_emb.weight'] - P64).max(),
                               np.abs(batch_tabs['item_emb.weight'] - Q64).max()))
    t_no, _, (P_no, _), _ = trajectory64(name, sels, with_term=False)
    print(f'g19 {name}: {len(sels)} steps, block at most {max(len(a) for a, _ in sels)} x {max(len(b) for _, b in sels)}; '
          f'reference vs float64: loss dicts max rel {dist_loss:.2e}, final tables max abs {dist_tab:.2e} '
          f'(scale {np.abs(P64).max():.2f}), first step {dist_first:.2e}, train_a_batch {dist_batch_loss:.2e} / '
          f'{dist_batch_tab:.2e}; without the term: losses {np.max(np.abs(traj - t_no) / np.abs(t_no)):.2e}, '
          f'tables {np.abs(final["user_emb.weight"] - P_no).max():.2e}')

    cap_u, cap_i = max(len(a) for a, _ in sels), max(len(b) for _, b in sels)
    su = np.zeros((len(sels), cap_u), np.int16)
    si = np.zeros((len(sels), cap_i), np.int16)
    for s, (a, b) in enumerate(sels):
        su[s, :len(a)], si[s, :len(b)] = a, b
    out = {'meta': np.array([U, I, D, n, bs, epochs]), 'cfg': np.array([cfg['lr'], cfg['L2_coe'], cfg['L1_coe']]),
           'seed': np.array(seed), 'sel_users': su, 'sel_items': si,
           'sel_nu': np.array([len(a) for a, _ in sels], np.int16), 'sel_ni': np.array([len(b) for _, b in sels], np.int16),
           'traj': traj, 'loss_epochs': np.array(loss_epochs), 'pairs': pairs,
           'batch_su': batch_sel[0].astype(np.int16), 'batch_si': batch_sel[1].astype(np.int16), 'batch_loss': batch_loss,
           'dist_loss_rel': np.array(dist_loss), 'dist_tab_abs': np.array(dist_tab), 'dist_first_abs': np.array(dist_first),
           'dist_batch_loss_rel': np.array(dist_batch_loss), 'dist_batch_tab_abs': np.array(dist_batch_tab),
           'zero_tensor_all_zero': np.array(True)}
    for k in final:
        out['first_' + k], out['final_' + k], out['batch_' + k] = first_tabs[k], final[k], batch_tabs[k]
    np.savez_compressed(os.path.join(HERE, f'g19_wmf_{name}.npz'), **out)


if __name__ == '__main__':
    torch.manual_seed(0)
    torch.set_num_threads(1)
    gen_block()
    for name in CASES:
        gen_case(name)
