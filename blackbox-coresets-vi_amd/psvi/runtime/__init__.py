"""MI355X runtime of the coreset-ELBO inner loop: ctypes boundary to libpsvi_hip.so."""
from ._lib import PsviError, load  # noqa: F401
from .engine import (InnerLoopPlan, adam_adjoint_, adam_update_, make_adam, nonfinite_,  # noqa: F401
                     randn_, check_binary, select_scores, select_weight_grad, laplace_fit,
                     laplace_sample_full, laplace_scores, giga_step, mfvi_fit, mfvi_fit_query, coreset_draw, predict_scores,
                     predict_query, kmeans, kmeans_query)
