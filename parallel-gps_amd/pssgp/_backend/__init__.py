"""ctypes binding of libpgps.so (include/pgps.h) -- the only way pssgp reaches the GPU.

There is no CPU fallback: if the library is missing or no MI355X is visible the calls raise.

This module only re-exports; `from pssgp import _backend` stays the one import.  Callers reach every entry point as
`_backend.NAME(...)` at call time, so a name patched here is the one the model layer sees.  Where each concern lives:
library (path, loading, the signature table, errors), context, arrays (input preparation shared by all calls), lgssm,
fused, lti, series, batch, sites (Laplace inference), panel (S series on their own clocks)."""
from .library import (COMM_ID_BYTES, E_NUMERIC, E_UNSUPPORTED_DIM, PGPS_K_NAMES, PGPS_OK, PgpsError, _LIB_PATH, _require, check,
                      load_library, signatures)
from .context import Context, _contexts, get_context
from .arrays import _prep, _ptr, _scalar_out, _series_inputs, _suffix
from .lgssm import _cov_inputs, _dtype_of, _sample_inputs, _unpack_lgssm, discretise, pkf, pkfs, pks, pks_cov, pks_sample
from .lti import (LTI_BATCH_DIM_MAX, LTI_DIM_MAX, LTI_DIM_MIN, LTI_FUNCTIONALS_MAX, LtiGradStream, LtiLlStream, _lti_model, contract_grad_stats, lti_ll,
                  lti_ll_grad, lti_predict, lti_predict_cov, lti_predict_lin, lti_predict_stream, lti_sample, split_grad_stats)
from .fused import (GRAD_BLOCKS_DIM_MAX, GRAD_BLOCKS_MAX, GRAM_COLUMNS_MAX, gp, gp_gram_multi, gp_ll_grad, gp_ll_grad_adj_het,
                    gp_ll_grad_blocks, gp_ll_grad_multi, gp_ll_het, gp_ll_multi, gp_loo, gp_predict, gp_predict_het,
                    gp_predict_multi, gp_whiten_multi, nilpotent_blocks, nilpotent_form, normal_log_density, pack_grad_model)
from .batch import (_gp_rows, _lti_table, gp_ll_batch, gp_ll_grad_adj_batch, gp_predict_batch, lti_ll_batch, lti_ll_grad_batch,
                    lti_predict_batch, mix_moments)
from .series import PackBuffer, Series, _Packed
from . import panel
from .panel import (NEWTON_MAX_ITER_CAP, PANEL_GRAM_COLUMNS_MAX, PANEL_INFO, PANEL_MAX_STEPS, PanelData, gp_panel_gram,
                    gp_panel_laplace, gp_panel_laplace_grad, gp_panel_ll, gp_panel_ll_grad, gp_panel_loo, gp_panel_predict,
                    gp_panel_trend_solve)
from .sites import (LIK_BERNOULLI_LOGIT, LIK_GAUSSIAN, LIK_POISSON_EXP, LIK_W_MIN, NEWTON_SUMS, SiteBuffers, gp_newton,
                    lik_sites)
