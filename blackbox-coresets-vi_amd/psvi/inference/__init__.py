"""Inner-loop surface of the reference's psvi.inference (PSVI classes)."""
from .psvi_classes import (PSVI, PSVIAV, PSVIAFixedU, PSVIFixedU, PSVIFreeV,  # noqa: F401
                           PSVILearnV, PSVI_Ablated, PSVI_No_IW, PSVI_No_Rescaling, HipInnerELBO,
                           PSVI_regressor, PSVILearnV_regressor, PSVIAV_regressor)
from .baselines import (run_mfvi, run_mfvi_subset, run_random, run_sparsevi,  # noqa: F401,E402
                        run_opsvi, run_giga, run_laplace, process_wt_index, fit,
                        run_mfvi_regressor, run_mfvi_subset_regressor, MfviSelect,
                        run_selection_with_mfvi)
from .utils import (MeanFieldVI, WeightedSubset, Selection, RandomSelection,  # noqa: F401,E402
                    ScoreSelection, RandomScoreSelection, ScoreCalculator, CoresetSelect,
                    KmeansCluster, KmeansSelection, KmeansScoreSelection,
                    WeightedKmeansSelection)
from .sparsebbvi import run_sparsevi_with_bb_elbo  # noqa: F401,E402
