"""colnde — MI355X-native NDE column-model hot path.

`import colnde` (alias module at the repo root) loads this package.  Host code is pure Python over the
C ABI of libcolnde.so; the HIP extension is mandatory (no CPU fallback)."""
from .config import (NDEConfig, ZeroMeanUnitVarianceScaling, WIND_MIXING, FREE_CONVECTION,
                     CONVECTIVE_ADJUSTMENT_NDE)
from . import flux_compat, synthetic
from ._lib import ColndeError, build as build_extension, LIB_PATH
from .nde import ColumnNDE, ColumnNDEEnsemble, TileNDEEnsemble, is_net_split_shape, FreeConvectionEnsemble, check_fc_ensemble_arrays, check_fc_pretrain_arrays, check_wm_pretrain_arrays, ClosureColumns, check_closure_arrays, check_fc_embed_arrays, check_wm_diag_arrays, check_wm_ens_embed_arrays, WmEnsembleEmbedded, check_wm_profile_arrays, EnsembleProfile,check_fc_ens_embed_arrays, FcEnsembleEmbedded, closure_min_substeps, min_substeps, rkc_stages, schedule_min
from . import distributed, wind_mixing, free_convection
