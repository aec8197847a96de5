"""enerf_event_c_estimate (csrc/event_pairs.hip: four masked medians by a radix select, one launch) against
event_diag.estimate_C_thres_statement -- the reference's function restated, held to the reference by
tests/test_c_estimate_host.py -- on the same inputs, the statement evaluated on the CPU.  Medians compare with ==
(NaN-aware; 0.0 == -0.0), counts exactly: a median is one of the class's quotients, and the quotient is the correctly
rounded fp32 one on both sides, so there is nothing to tolerate."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (50001: more than one round of the kernel's load loop -- a thread takes up to 24 events per round -- at every C)
NS = [1, 2, 4, 5, 63, 64, 65, 1023, 1024, 1025, 4097, 20096, 50001]


def _signs(g, n):
    return torch.where(torch.rand(n, generator=g) < 0.5, 1.0, -1.0)


def _bits(x):
    return x.to(torch.int32).view(torch.float32)


def _value_sets(n, C, seed):
    """name -> (pols [n,1], delta [n,C]) on the CPU: inputs chosen to break a radix select."""
    g = torch.Generator().manual_seed(seed)
    sets = {}
    sets["random"] = (_signs(g, n), torch.randn(n, C, generator=g))
    # every key in one bin on every pass
    sets["all_equal"] = (_signs(g, n), torch.full((n, C), 0.375))
    sets["all_zero"] = (_signs(g, n), torch.zeros(n, C))
    # the first three passes cannot tell the values apart
    sets["low_8_bits"] = (_signs(g, n), _bits(0x3F000000 + torch.randint(0, 256, (n, C), generator=g)))
    # mixed signs around +-0
    lv = torch.tensor([-1.0, -0.0, 0.0, 1.0, -1e-30, 1e-30, 0.5])
    sets["signs_and_zeros"] = (_signs(g, n) * torch.randint(1, 3, (n,), generator=g),
                               lv[torch.randint(0, len(lv), (n, C), generator=g)])
    den = _bits(torch.randint(1, 1 << 20, (n, C), generator=g)) * _signs(g, n)[:, None]
    sets["denormals"] = (_signs(g, n) * 2.0 ** torch.randint(0, 3, (n,), generator=g).float(), den)
    d = torch.randn(n, C, generator=g)
    d[torch.rand(n, C, generator=g) < 0.3] = float("inf")
    d[torch.rand(n, C, generator=g) < 0.3] = float("-inf")
    sets["infinities"] = (_signs(g, n), d)
    # a NaN in the last channel of a positive event: in the classes that event is in
    p, d = _signs(g, n), torch.randn(n, C, generator=g)
    p[n // 2] = 1.0
    d[n // 2, C - 1] = float("nan")
    sets["nan_in_a_class"] = (p, d)
    # a NaN only in channel 0: fails both sign conditions
    p, d = _signs(g, n), torch.randn(n, C, generator=g)
    d[n // 3, 0] = float("nan")
    sets["nan_in_channel_0"] = (p, d)
    p = -torch.ones(n)
    p[n - 1] = 3.0
    sets["one_positive_event"] = (p, torch.randn(n, C, generator=g))
    sets["every_event_positive"] = (torch.full((n,), 2.0), torch.randn(n, C, generator=g))
    sets["every_event_negative"] = (torch.full((n,), -0.5), torch.randn(n, C, generator=g).abs())
    sets["zero_polarities"] = (torch.randint(-1, 2, (n,), generator=g).float(), torch.randn(n, C, generator=g))
    sets["accumulated"] = (torch.randint(-4, 5, (n,), generator=g).float(), 0.3 * torch.randn(n, C, generator=g))
    # mostly ties, as early in training
    d = 0.1 * torch.randn(n, C, generator=g)
    d[torch.rand(n, generator=g) < 0.8] = 0.0
    sets["mostly_zero"] = (_signs(g, n), d)
    return {k: (p.reshape(n, 1).contiguous(), d.contiguous()) for k, (p, d) in sets.items()}


def _want(pols, delta):
    from enerf_amd.event_diag import NAMES, estimate_C_thres_statement
    est, counts = estimate_C_thres_statement(pols, delta, with_counts=True)
    return np.array([float(est[k]) for k in NAMES], np.float32), counts


def _same(got, want):
    return bool(np.all((got == want) | (np.isnan(got) & np.isnan(want))))


@pytest.mark.parametrize("C", [1, 2, 3])
@pytest.mark.parametrize("n", NS)
def test_kernel_equals_the_statement(n, C):
    from enerf_amd import _lib as L
    from enerf_amd.event_diag import estimate_C_thres
    lib = L.lib()
    calls = []
    orig = lib.enerf_event_c_estimate
    lib.enerf_event_c_estimate = lambda *a: (calls.append(a[2:4]), orig(*a))[1]
    try:
        for name, (pols, delta) in _value_sets(n, C, 1000 * C + n).items():
            want, counts = _want(pols, delta)
            p, d = pols.to(DEV), delta.to(DEV)
            med, cnt = estimate_C_thres(p, d)
            med2, cnt2 = estimate_C_thres(p[:, 0][None], d[None])            # the event step's layout, a second run
            got = med.cpu().numpy()
            print(f"n={n} C={C} {name}: got {got} want {want} counts {cnt.tolist()}")
            assert med.device.type == "cuda" and med.dtype == torch.float32 and cnt.dtype == torch.int32
            assert cnt.tolist() == counts, (name, cnt.tolist(), counts)
            assert _same(got, want), (name, got, want)
            # the same bits on every run
            assert torch.equal(med.view(torch.int32), med2.view(torch.int32)) and torch.equal(cnt, cnt2), name
    finally:
        lib.enerf_event_c_estimate = orig
    assert calls and set(calls) == {(n, C)} and len(calls) == 2 * len(_value_sets(1, 1, 0))     # one launch per call


def test_three_events_take_the_statement_and_its_luma():
    """N == 3: the reference forms a luma of the three EVENTS' rows; the kernel is not asked."""
    from enerf_amd import _lib as L
    from enerf_amd.event_diag import estimate_C_thres
    lib = L.lib()
    calls = []
    orig = lib.enerf_event_c_estimate
    lib.enerf_event_c_estimate = lambda *a: (calls.append(1), orig(*a))[1]
    try:
        pols, delta = torch.tensor([[1.0], [-1.0], [1.0]]), torch.tensor([[0.3, 0.1, -0.2], [0.5, -0.4, 0.1], [-0.1, 0.2, 0.6]])
        med, cnt = estimate_C_thres(pols.to(DEV), delta.to(DEV))
    finally:
        lib.enerf_event_c_estimate = orig
    want, counts = _want(pols, delta)
    assert not calls and med.device.type == "cuda" and cnt.tolist() == counts == [2, 1, 2, 1]
    assert np.allclose(med.cpu().numpy(), want, rtol=1e-6, atol=0)           # (the luma's sum on the device: round-off)


def test_writes_into_a_row_and_does_not_synchronise():
    from enerf_amd.event_diag import estimate_C_thres
    pols, delta = _value_sets(4097, 3, 5)["accumulated"]
    want, counts = _want(pols, delta)
    p, d = pols.to(DEV)[:, 0][None].contiguous(), delta.to(DEV)[None].contiguous()
    ring = torch.full((3, 12), -7.0, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        raised = False
        try:
            torch.ones(1, device=DEV).item()
        except RuntimeError:
            raised = True
        if raised:                                # (else: this torch build does not police synchronisation)
            estimate_C_thres(p, d, out=ring[1, 4:])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not raised:
        print("sync debug mode does not raise on .item() in this torch build: the no-synchronisation check did not run")
        estimate_C_thres(p, d, out=ring[1, 4:])
    host = ring.cpu()
    assert _same(host[1, 4:8].numpy(), want) and host[1, 8:].contiguous().view(torch.int32).tolist() == counts
    assert bool((host[0] == -7).all() and (host[2] == -7).all() and (host[1, :4] == -7).all())


def test_refusals_and_the_empty_input():
    from enerf_amd import _lib as L
    lib = L.lib()
    d, p = torch.randn(8, 3, device=DEV), torch.ones(8, device=DEV)
    med = torch.full((4,), 5.0, device=DEV)
    cnt = torch.full((4,), 9, dtype=torch.int32, device=DEV)
    s = L.stream_handle()
    for ch in (0, 4):
        assert lib.enerf_event_c_estimate(d.data_ptr(), p.data_ptr(), 8, ch, med.data_ptr(), cnt.data_ptr(), s) == -1
    assert lib.enerf_event_c_estimate(None, p.data_ptr(), 8, 3, med.data_ptr(), cnt.data_ptr(), s) == -1
    assert lib.enerf_event_c_estimate(d.data_ptr(), None, 8, 3, med.data_ptr(), cnt.data_ptr(), s) == -1
    assert lib.enerf_event_c_estimate(d.data_ptr(), p.data_ptr(), 8, 3, None, cnt.data_ptr(), s) == -1
    assert b"event_c_estimate" in lib.enerf_last_error()
    torch.cuda.synchronize()
    assert med.tolist() == [5.0] * 4 and cnt.tolist() == [9] * 4             # a refused call writes nothing
    # N == 0: four zeros and zero counts, with or without inputs
    L.check(lib.enerf_event_c_estimate(None, None, 0, 1, med.data_ptr(), cnt.data_ptr(), s), "event_c_estimate")
    assert med.tolist() == [0.0] * 4 and cnt.tolist() == [0] * 4
    # counts may be NULL
    L.check(lib.enerf_event_c_estimate(d.data_ptr(), p.data_ptr(), 8, 3, med.data_ptr(), None, s), "event_c_estimate")
    want, _ = _want(p.cpu()[:, None], d.cpu())
    assert _same(med.cpu().numpy(), want)
