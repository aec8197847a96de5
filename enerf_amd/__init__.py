"""enerf_amd -- MI355X (gfx950) implementation of the instant-ngp hot path under knelk/enerf.

Layout
  csrc/        hand-written HIP kernels + the C ABI (include/enerf_hip.h) -> lib/libenerf_hip.so
  backends/    ctypes shims with the reference's pybind module/function names (_raymarching, _gridencoder, ...)
  ext/         pybind11 modules of the same four names over the C ABI, importable as top-level `_raymarching` ... by the
               reference's untouched Python wrappers
  raymarching, gridencoder, shencoder, ffmlp      host-side mirror of the reference's autograd wrappers
  encoding, activation, renderer, network, network_ff, events   the callers re-stated for the bench harness
  optim, parallel                                  fused optimizer + ray-sharded data parallel step

There is no CPU fallback in this package: every hot-path call goes to libenerf_hip.so or raises.
"""
__version__ = "0.1.0"

# the data-side entry points and the view renderer, resolved on first use (importing the package stays free of torch)
_EXPORTS = {"FrameSampler": "frame_sampler", "EventSampler": "event_sampler", "ViewRenderer": "view",
            "interpolate_poses": "render_path", "spiral_poses": "render_path", "poses_from_quat_list": "render_path"}
__all__ = sorted(_EXPORTS)


def __getattr__(name):
    if name in _EXPORTS:
        import importlib
        return getattr(importlib.import_module("." + _EXPORTS[name], __name__), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
