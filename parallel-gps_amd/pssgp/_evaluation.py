"""Decorators of StateSpaceGP's public evaluations: counting them, and refusing what a model does not cover."""
import functools


def _public_evaluation(fn):
    """Marks the model's public evaluations (predict_f, maximum_log_likelihood_objective, log_likelihood_and_grad,
    log_likelihood_batch).  `_device_series()` counts THESE -- the outermost one of a call chain -- not its own calls: one
    evaluation may ask for the series several times on its way through the gradient methods and must get the same answer
    each time (round 4 counted calls: the first gradient of a Matern model got None for its fused adjoint, a series on
    the next internal call, and went down the dual-number road it had not chosen)."""
    @functools.wraps(fn)
    def wrapper(self, *args, **kwargs):
        depth = getattr(self, "_eval_depth", 0)
        if depth == 0:
            self._n_eval = getattr(self, "_n_eval", 0) + 1
        self._eval_depth = depth + 1
        try:
            return fn(self, *args, **kwargs)
        finally:
            self._eval_depth = depth
    return wrapper


def _single_output_evaluation(fn):
    """A public evaluation that exists for one output column and one shared noise variance only (the batches and the
    draws).  The order of effects: NotImplementedError for num_latent_gps > 1 BEFORE the evaluation is counted, then the
    count (_public_evaluation), then NotImplementedError when observation_variances is set."""
    @_public_evaluation
    @functools.wraps(fn)
    def counted(self, *args, **kwargs):
        if self._obs_var is not None:
            raise NotImplementedError(f"{fn.__name__} is not available with observation_variances set (per-observation noise "
                                      "variances cover maximum_log_likelihood_objective, predict_f and log_likelihood_and_grad)")
        return fn(self, *args, **kwargs)

    @functools.wraps(fn)
    def wrapper(self, *args, **kwargs):
        if self.num_latent_gps > 1:
            raise NotImplementedError(f"{fn.__name__} covers single-output models; this one has {self.num_latent_gps} output columns")
        return counted(self, *args, **kwargs)
    return wrapper


def _multi_output(route):
    """A model with num_latent_gps > 1 answers this evaluation with its method `route`; a single-output model runs the decorated
    function exactly as before."""
    def deco(fn):
        @functools.wraps(fn)
        def wrapper(self, *args, **kwargs):
            if self.num_latent_gps > 1:
                return getattr(self, route)(*args, **kwargs)
            return fn(self, *args, **kwargs)
        return wrapper
    return deco


def _mean_function_route(route):
    """A model with a mean_function answers this evaluation with its method `route` (trend.py: delegation to the zero-mean model
    on the residuals); a model without one runs the decorated function exactly as before."""
    def deco(fn):
        @functools.wraps(fn)
        def wrapper(self, *args, **kwargs):
            if self._mean_function is not None:
                return getattr(self, route)(*args, **kwargs)
            return fn(self, *args, **kwargs)
        return wrapper
    return deco


def _zero_mean_evaluation(fn):
    """A public evaluation whose `thetas` layout has no place for the mean function's coefficients (the batches)."""
    @functools.wraps(fn)
    def wrapper(self, *args, **kwargs):
        if self._mean_function is not None:
            raise NotImplementedError(f"{fn.__name__} is not available with a mean_function set")
        return fn(self, *args, **kwargs)
    return wrapper
