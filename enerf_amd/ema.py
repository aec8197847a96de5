"""`ParamEMA`: the exponential moving average of a model's parameters, as the reference's Trainer keeps one
(nerf/utils.py:370-371 `ExponentialMovingAverage(self.model.parameters(), decay=ema_decay)`, main_nerf.py:214
`ema_decay=0.95`): updated once per epoch (nerf/utils.py:1005-1006), swapped in around every evaluation (:1041-1043,
1290-1291) and for the "best" checkpoint (:1339-1347), stored under 'ema' in a full checkpoint (:1314-1315, 1379-1380).

This is `torch_ema.ExponentialMovingAverage` as the reference calls it, RESTATED here from that library's release 0.3
(its documented behaviour and state-dict format), because the library itself is not available where this project is
built and tested; nothing of it is imported.  What is restated:

    shadow_params    detached clones of EVERY parameter, in the order given
    update()         num_updates += 1; decay = min(decay, (1 + num_updates) / (10 + num_updates)) in Python doubles;
                     omd = 1.0 - decay; per tensor  tmp = s - p; tmp.mul_(omd); s.sub_(tmp)
    store / copy_to / restore      clone the parameters / shadow -> parameters / the clones -> parameters
    state_dict()     {"decay", "num_updates", "shadow_params": [...], "collected_params": None or [...]}

The update's arithmetic per element is  s = s - ((s - p) * fp32(omd)):  three fp32 operations, each rounded once (torch
casts the Python scalar to the tensor's dtype).  CUDA fp32 contiguous tensors take it in ONE launch per 16 tensors
(csrc/optim.hip k_ema_multi, enerf_ema_update_multi: 12 B/parameter, no temporary, no allocation, no synchronisation,
on the caller's current stream); everything else takes `ema_statement`, which is also what the tests hold the kernel to.

store / copy_to / restore copy IN PLACE and never exchange `.data`: the one-call steps and FusedAdam cache the
parameters' device pointers.  
"""
import ctypes

import torch

from . import _lib as L

MAX_TENSORS = 16                # csrc/optim.hip kMaxAdamTensors


def ema_statement(shadow, param, omd):
    """torch_ema's update of one tensor, in place on `shadow`: tmp = s - p; tmp.mul_(omd); s.sub_(tmp)."""
    with torch.no_grad():
        tmp = shadow - param
        tmp.mul_(omd)
        shadow.sub_(tmp)
    return shadow


def _native(s, p):
    return (s.is_cuda and p.is_cuda and s.device == p.device and s.dtype == torch.float32 and p.dtype == torch.float32
            and s.is_contiguous() and p.is_contiguous() and s.numel() == p.numel())


def ema_update_multi(shadows, params, omd):
    """enerf_ema_update_multi over CUDA fp32 contiguous tensors of one device, in calls of at most 16 tensors."""
    for k in range(0, len(shadows), MAX_TENSORS):
        s, p = shadows[k:k + MAX_TENSORS], params[k:k + MAX_TENSORS]
        n = len(s)
        vp, sz = ctypes.c_void_p * n, ctypes.c_size_t * n
        L.check(L.lib().enerf_ema_update_multi(n, vp(*[t.data_ptr() for t in s]), vp(*[t.data_ptr() for t in p]),
                                               sz(*[t.numel() for t in s]), omd, L.stream_handle()),
                "ema_update_multi")


class ParamEMA:
    def __init__(self, parameters, decay, use_num_updates=True):
        if decay < 0.0 or decay > 1.0:
            raise ValueError("Decay must be between 0 and 1")
        self.decay = decay
        self.num_updates = 0 if use_num_updates else None
        self.parameters = list(parameters)
        self.shadow_params = [p.clone().detach() for p in self.parameters]
        self.collected_params = None

    def _get_parameters(self, parameters):
        if parameters is None:
            return self.parameters
        parameters = list(parameters)
        if len(parameters) != len(self.shadow_params):
            raise ValueError("Number of parameters passed as argument is different from number of shadow parameters "
                             "maintained by this ExponentialMovingAverage")
        return parameters

    def update(self, parameters=None):
        """One step of the average towards the parameters' current values."""
        parameters = self._get_parameters(parameters)
        decay = self.decay
        if self.num_updates is not None:
            self.num_updates += 1
            decay = min(decay, (1 + self.num_updates) / (10 + self.num_updates))
        omd = 1.0 - decay
        native = {}                                     # device -> (shadows, parameters) the kernel takes
        for s, p in zip(self.shadow_params, parameters):
            if _native(s, p):
                pair = native.setdefault(s.device, ([], []))
                pair[0].append(s)
                pair[1].append(p.detach())
            else:
                ema_statement(s, p.detach(), omd)
        for dev, (ss, ps) in native.items():
            if dev.index is not None and dev.index != torch.cuda.current_device():
                with torch.cuda.device(dev):
                    ema_update_multi(ss, ps, omd)
            else:
                ema_update_multi(ss, ps, omd)

    def store(self, parameters=None):
        """Keep a copy of the parameters' current values for restore()."""
        parameters = self._get_parameters(parameters)
        self.collected_params = [p.detach().clone() for p in parameters]

    def copy_to(self, parameters=None):
        """The average -> the parameters, in place."""
        parameters = self._get_parameters(parameters)
        with torch.no_grad():
            for s, p in zip(self.shadow_params, parameters):
                p.copy_(s)

    def restore(self, parameters=None):
        """What store() kept -> the parameters, in place."""
        if self.collected_params is None:
            raise RuntimeError("This ExponentialMovingAverage has no `store()`ed weights to `restore()`")
        parameters = self._get_parameters(parameters)
        with torch.no_grad():
            for c, p in zip(self.collected_params, parameters):
                p.copy_(c)

    def state_dict(self):
        """The dict the reference stores under 'ema' (tensors, numbers, lists and None)."""
        return {"decay": self.decay, "num_updates": self.num_updates, "shadow_params": self.shadow_params,
                "collected_params": self.collected_params}

    def load_state_dict(self, state_dict):
        decay = state_dict["decay"]
        if decay < 0.0 or decay > 1.0:
            raise ValueError("Decay must be between 0 and 1")
        num_updates = state_dict["num_updates"]
        if not (num_updates is None or (isinstance(num_updates, int) and not isinstance(num_updates, bool))):
            raise ValueError("Invalid num_updates")
        shadow = state_dict["shadow_params"]
        if not isinstance(shadow, list) or not all(torch.is_tensor(t) for t in shadow):
            raise ValueError("shadow_params must be a list of Tensors")
        collected = state_dict.get("collected_params")
        if collected is not None:
            if not isinstance(collected, list) or not all(torch.is_tensor(t) for t in collected):
                raise ValueError("collected_params must be a list of Tensors")
            if len(collected) != len(shadow):
                raise ValueError("collected_params and shadow_params had different lengths")
        params = self.parameters
        if len(shadow) != len(params):
            raise ValueError("Tried to `load_state_dict()` with the wrong number of parameters in the saved state.")
        for group in (shadow, collected or []):
            for t, p in zip(group, params):
                if tuple(t.shape) != tuple(p.shape):
                    raise ValueError(f"Tried to `load_state_dict()` with a tensor of shape {tuple(t.shape)} for a "
                                     f"parameter of shape {tuple(p.shape)}")

        def onto(ts):
            return [t.detach().to(device=p.device, dtype=p.dtype, copy=True) for t, p in zip(ts, params)]
        self.decay, self.num_updates = decay, num_updates
        self.shadow_params = onto(shadow)
        self.collected_params = None if collected is None else onto(collected)
