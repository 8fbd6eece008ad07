"""InvPref (KDD 2022) and its PureMF baselines on hand-written HIP kernels for gfx950."""

_FAIRNESS = ('FairnessMFTrainManager', 'fairness_item_table', 'fairness_draw', 'fairness_draw_epochs')

_MACR = ('MACRMatrixFactorization', 'MACRTrainManager')

_LINTRANS = ('LinearTransMatrixFactorization', 'LinearTransTrainManager')

_CAUSE = ('CausEMatrixFactorization', 'CausEExplicitMatrixFactorization', 'CausETrainManager', 'CausEExplicitTrainManager')

_BPR = ('BPRTrainManager',)

_DR = ('DRMatrixFactorization', 'DRExplicitMatrixFactorization', 'DRTrainManager', 'DRExplicitTrainManager')

_ALS = ('ALSTrainManager',)

_SSM = ('SSMTrainManager',)

_LGCN = ('LightGCNMatrixFactorization', 'LightGCNTrainManager')

_DICE = ('DICEMatrixFactorization', 'DICETrainManager')

_EASE = ('EASEModel', 'EASETrainManager')
_MULTDAE = ('MultDAEModel', 'MultDAETrainManager')

_EVALUATE = ('ExplicitRankTestManager',)


def __getattr__(name):   # resolved on first use: importing the package loads neither torch nor the HIP library
    if name in _EVALUATE:
        from . import evaluate
        return getattr(evaluate, name)
    if name in _FAIRNESS or name in _MACR or name in _LINTRANS or name in _CAUSE or name in _BPR or name in _DR \
            or name in _ALS or name in _SSM or name in _LGCN or name in _DICE or name in _EASE or name in _MULTDAE:
        from . import baseline
        return getattr(baseline, name)
    raise AttributeError(f'module {__name__!r} has no attribute {name!r}')
