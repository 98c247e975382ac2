"""
MI355X-native Muskingum routing engine behind river-route's Router API.

    import river_route_amd as rr
    rr.RapidMuskingum('config.yaml').route()

mirrors `import river_route as rr` of the reference for the routing hot path (river_route/__init__.py:11-29):
Configs, Muskingum, RapidMuskingum, UnitMuskingum, uhkernels.UnitHydrograph, runoff.runoff_to_qlateral, runoff.grid_weights, tools.adjacency_matrix, metrics, and grad (torch autograd through the engine: calibration of k and x).  The compute
runs in hand-written HIP kernels (csrc/, C ABI in include/rr_hip.h); there is no CPU fallback.
"""
__version__ = '0.1.0'

from . import metrics, runoff, synth, tools, uhkernels  # noqa: E402
from .routers import Configs, Muskingum, RapidMuskingum, UnitMuskingum  # noqa: E402

__all__ = ['Configs', 'Muskingum', 'RapidMuskingum', 'UnitMuskingum', 'uhkernels', 'runoff', 'tools', 'synth', 'metrics', 'grad', '__version__']


def __getattr__(name):
    # rr.grad imports torch: loaded on first use, so `import river_route_amd` stays as light as it was
    if name == 'grad':
        import importlib
        return importlib.import_module('.grad', __name__)
    raise AttributeError(f'module {__name__!r} has no attribute {name!r}')
