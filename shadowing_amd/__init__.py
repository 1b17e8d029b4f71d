"""shadowing_amd -- the k-nearest-path scan of Path Shadowing Monte-Carlo on MI355X.

One hot path of RudyMorel/shadowing, rebuilt MI355X-first: PathShadowing.shadow()
with Identity + RelativeMSE + PredictionContext runs as hand-written gfx950 HIP
kernels behind the reference's own PathShadowing / PathEmbedding / PathDistance /
context plugin surface (a drop-in for that path and nothing else).
"""
from .averaging import DiscreteProba, Softmax, Uniform
from .path_distance import PathDistance, RelativeMSE
from .path_embedding import (ArrayType, ContextManagerBase, CrossChannelContext, Foveal, Identity,
                             ImputationContext, PathEmbedding, PredictionContext)
from .path_shadowing import PathShadowing, PendingShadow, select_cartesian_product
from .plotting import plot_closest, plot_shadow, plot_volatility
from .mrw import (MRWGenerator, SMRWGenerator, mrw_log_returns, smrw_kernel, smrw_leverage, smrw_log_returns,
                  smrw_sq_moment)
from .pdv import AutoregressiveLinearPredictor, PDVModel, PDVModelDiscrete
from .pricing import HedgedPnL, HedgePolicy, PriceData, Smile, compute_smile, hedge_pnl
from .quantiles import PredictiveQuantiles, weighted_quantiles
from .scoring import EnsembleScore, score_ensemble
from .statistics import realized_variance
from .weights import softmax_weights
from .separation import Separated, separate_topk
from .calibration import Calibration, MarketQuotes, calibrate_host, calibrate_weights
from .stylized import LaggedMoments, fit_smrw, lagged_moments
from .scattering import (ScatteringSpectra, scattering_bank, scattering_generate, scattering_loss, scattering_spectra,
                         scattering_sums)

__all__ = [
    "ArrayType", "ContextManagerBase", "PredictionContext", "ImputationContext", "CrossChannelContext",
    "PathEmbedding", "Identity", "Foveal", "PathDistance", "RelativeMSE", "PathShadowing",
    "select_cartesian_product", "DiscreteProba", "Softmax", "Uniform", "realized_variance",
    "plot_closest", "plot_shadow", "plot_volatility", "PriceData", "Smile", "compute_smile", "hedge_pnl", "HedgePolicy", "HedgedPnL",
    "PDVModel", "PDVModelDiscrete", "AutoregressiveLinearPredictor",
    "MRWGenerator", "mrw_log_returns", "SMRWGenerator", "smrw_log_returns", "smrw_kernel", "smrw_leverage",
    "smrw_sq_moment", "LaggedMoments", "lagged_moments", "fit_smrw",
    "ScatteringSpectra", "scattering_spectra", "scattering_bank", "scattering_sums", "scattering_loss",
    "scattering_generate", "PredictiveQuantiles", "weighted_quantiles", "EnsembleScore", "score_ensemble",
    "softmax_weights", "Separated", "separate_topk", "Calibration", "MarketQuotes", "calibrate_weights", "calibrate_host",
]
__version__ = "0.1.0"
