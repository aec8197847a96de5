"""Host checks of tests/composite_ref.py (no GPU): the closed-form gradients of the fp64 reference against autograd on the
plain definition; the C oracle (fp32, sequential, three channels) and a numpy fp32 statement of the kernels' scan order
under the very bars the GPU test uses -- the evidence that the bars are not too tight for correct fp32 arithmetic; every
seeded defect of that statement rejected by the comparator, on a named case; and the conditions on the inputs."""
import functools

import numpy as np
import pytest
import torch

import composite_ref as R

ALL = list(range(R.N_CASES))
FORMS = ["plain", "mse", "frames", "frames_alpha"]


# ------------------------------------------------------------------------------------------------- reference against autograd
def _autograd(c, form, out_ref):
    """d sigma, d rgb of the plain definition by torch.autograd in float64 (marched rays only; others stay NaN / 0)."""
    N = c["N"]
    sig = torch.tensor(c["sigmas"], dtype=torch.float64, requires_grad=True)
    rgb = torch.tensor(c["rgbs"], dtype=torch.float64, requires_grad=True)
    dl = torch.tensor(c["deltas"], dtype=torch.float64)
    bg = torch.tensor(c["bg_rows"], dtype=torch.float64)
    g, gws, _, _, weight = R.upstream(c, form, out_ref)
    loss = torch.zeros((), dtype=torch.float64)
    for n in range(N):
        idx, off, cnt = (int(v) for v in c["rays"][n])
        if not R.marched(c, n):
            continue
        x = sig[off:off + cnt] * dl[off:off + cnt, 0]
        alpha = -torch.expm1(-x)
        w = alpha * torch.exp(-(torch.cumsum(x, 0) - x))
        ws, image = w.sum(), (w[:, None] * rgb[off:off + cnt]).sum(0)
        if form == "plain":
            loss = loss + (torch.tensor(g[idx]) * image).sum() + float(gws[idx]) * ws
        else:
            out = image + (1.0 - ws) * bg[idx]
            if form == "mse":
                tgt, sc = torch.tensor(c["target"][idx], dtype=torch.float64), c["grad_scale"]
            else:
                tgt, sc = torch.tensor(R.frame_gt(c, form == "frames_alpha")[0][idx]), c["frame_scale"] * weight
            # d/d out of sc/2 * (out - tgt)^2 is sc * (out - tgt) -- at out == out_ref, which is where g was formed
            loss = loss + 0.5 * sc * ((out - tgt) ** 2).sum()
    loss.backward()
    return sig.grad.numpy(), rgb.grad.numpy()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("i", [1, 2, 3, 9, 11, 14])
def test_closed_form_gradients_agree_with_autograd(i, form):
    c = R.make_case(i)
    fwd, _ = R.forward_reference(i)
    ref = R.gradient_reference(i, form, fwd["out"][0])
    ags, agr = _autograd(c, form, fwd["out"][0])
    for (want, _), got, name in ((ref["gs"], ags, "d sigma"), (ref["gr"], agr, "d rgb")):
        own = np.isfinite(want)                      # plain form: rows no marched ray owns are NaN in the reference
        assert not got[~own].any()
        scale = np.abs(got[own]).max()
        err = np.abs(want[own] - got[own]).max()
        print(f"case {i} {form}: {name} max |closed form - autograd| = {err:.3g} on a scale of {scale:.3g}")
        assert scale > 0 and err <= 1e-12 * scale


# ------------------------------------------------------------------------------------------- the C oracle under the same bars
@functools.lru_cache(maxsize=None)
def _oracle_worst():
    from oracle import oracle as O
    W = R.Worst()
    for i in ALL:
        c = R.make_case(i, 3)
        rows, by_id = R.row_families(c)
        fwd, _ = R.forward_reference(i, 3)
        ws, depth, image = O.composite_rays_train_forward(c["sigmas"], c["rgbs"], c["deltas"], c["rays"])
        for name, got in (("ws", ws), ("depth", depth), ("image", image)):
            W.compare(f"oracle case {i}", name, fwd[name], got, by_id)
        out = (image + ((R.F32(1.0) - ws)[:, None] * c["bg_rows"]).astype(R.F32)).astype(R.F32)   # the blend, as torch rounds it
        W.compare(f"oracle case {i}", "out", fwd["out"], out, by_id)
        gs, gr = O.composite_rays_train_backward(c["g_ws"], c["g_image"], c["sigmas"], c["rgbs"], c["deltas"], c["rays"], ws,
                                                 image)
        ref = R.gradient_reference(i, "plain", C=3)
        unowned = np.isnan(ref["gs"][0])                 # the oracle's wrapper allocates zeroed buffers itself: no sentinel there
        assert not gs[unowned].any() and not gr[unowned].any()
        gs[unowned], gr[unowned] = np.nan, np.nan
        W.compare(f"oracle case {i}", "grad_sigmas", ref["gs"], gs, rows)
        W.compare(f"oracle case {i}", "grad_rgbs", ref["gr"], gr, rows)
    return W


def test_the_c_oracle_passes_the_same_bars():
    W = _oracle_worst()
    print(W.report("C oracle (fp32, sequential, C = 3), every family at every count:"))
    assert not W.fails, "\n".join(W.fails)
    assert {f for _, f in W.worst} >= set(R.FAMILIES) | {R.EMPTY, R.DROPPED}


# ------------------------------------------------------------------------- the scan-order statement and its seeded defects
@functools.lru_cache(maxsize=None)
def _statement(i, form, defect=None, weight=R.W03):
    return R.kernel_statement(i, form, defect, weight)


def _statement_worst(i, form, defect=None):
    W = R.Worst()
    one = _statement(i, form, None, 1.0) if form.startswith("frames") else None
    R.check_run(W, f"statement case {i} {form}" + (f" with {defect}" if defect else ""), i, form, _statement(i, form, defect),
              one)
    return W


@pytest.mark.parametrize("form", FORMS)
def test_the_scan_order_statement_passes_the_same_bars(form):
    worst = R.Worst()
    for i in ALL:
        W = _statement_worst(i, form)
        assert not W.fails, "\n".join(W.fails)
        for k, v in W.worst.items():
            worst.worst[k] = max(worst.worst.get(k, 0.0), v)
    print(worst.report(f"numpy fp32 statement of the scan order, {form}:"))


# where each seeded defect must be rejected: (case, form, output).  A defect may fail elsewhere too; it must fail here.
REJECTED_AT = {
    "no_T_carry": (6, "plain", "ws"),
    "no_colour_carry": (6, "plain", "image"),
    "no_ws_carry": (6, "plain", "ws"),
    "Tpre_in_dsigma": (4, "plain", "grad_sigmas"),
    "delta1_in_alpha": (3, "plain", "ws"),
    "no_delta0_in_dsigma": (3, "mse", "grad_sigmas"),
    "bg_sign": (4, "mse", "grad_sigmas"),
    "weight_folded_into_g": (6, "frames_alpha", "grad_sigmas vs weight 1"),
    "no_row_bcast15": (3, "plain", "ws"),
    "drop_rule_gt": (2, "mse", "out"),
}


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_every_seeded_defect_is_rejected(defect):
    i, form, output = REJECTED_AT[defect]
    W = _statement_worst(i, form, defect)
    bad = {o: v for o, v in W.per_output().items() if not v < 1.0}
    print(f"{defect}: rejected on case {i} ({form}) at " + ", ".join(f"{o} (error / bar = {v:.3g})" for o, v in bad.items()))
    assert output in bad, f"{defect} passes {output} of case {i} ({form}): the bar is too loose\n" + W.report("")
    assert not _statement_worst(i, form).fails


def test_the_defect_list_is_the_issues():
    assert sorted(REJECTED_AT) == sorted(R.DEFECTS) and len(R.DEFECTS) == 10


# ---------------------------------------------------------------------------------------------------- conditions on the inputs
def test_every_family_occurs_at_every_count_in_both_channel_settings():
    for C in (None, 3):
        seen = set()
        for i in ALL:
            c = R.make_case(i, C)
            assert c["M"] < 10000 and c["N"] == R.NS[i % 8]
            assert sorted(c["rays"][:, 0]) == list(range(c["N"]))
            for n in range(c["N"]):
                seen.add((c["fam"][n], int(c["rays"][n, 2])))
        assert seen >= {(f, n) for f in R.FAMILIES for n in R.COUNTS}
    assert {R.make_case(i)["C"] for i in ALL} == {1, 2, 3}
    assert {(R.make_case(i)["C"], R.make_case(i)["form"]) for i in ALL} >= {(C, f) for C in (1, 2, 3) for f in ("scalar", "ray")}
    assert {R.make_case(i)["N"] for i in ALL} == set(R.NS)


def test_walls_reach_exact_zero_and_thin_rays_stay_thin_in_fp32():
    wall = thin = 0
    for i in ALL:
        c = R.make_case(i)
        for n in range(c["N"]):
            _, off, cnt = (int(v) for v in c["rays"][n])
            s, d0 = c["sigmas"][off:off + cnt], c["deltas"][off:off + cnt, 0]
            alpha = R.F32(1.0) - np.exp(-(s * d0)).astype(R.F32)
            if c["fam"][n] == "WALL":
                assert np.multiply.accumulate((R.F32(1.0) - alpha).astype(R.F32))[-1] == 0.0 and (alpha == 1.0).any()
                wall += cnt > 2 and alpha[0] == 0.0          # the product hits zero mid-ray, not at its first sample
            if c["fam"][n] == "THIN":
                thin += bool((alpha < 1e-5).all() and (s > 0).all())
            if c["fam"][n] == "SAT_LATE" and cnt > 64:
                assert np.argmax(alpha) >= 64
    assert wall >= 10 and thin >= 3


def test_dropped_reservations_overlap_the_unreserved_tail():
    exact = past = 0
    for i in ALL:
        c = R.make_case(i)
        for n in range(c["N"]):
            _, off, cnt = (int(v) for v in c["rays"][n])
            if c["fam"][n] == R.DROPPED:
                assert off < c["counter"] < c["M"] <= off + cnt and not R.marched(c, n)
                exact += off + cnt == c["M"]
                past += off + cnt > c["M"]
            else:
                assert cnt == 0 or R.marched(c, n)
        assert c["counter"] <= c["M"] - 1
    assert exact >= 4 and past >= 4


# ------------------------------------------------------------------------------------------------------ inference compositing
def test_inference_rays_stay_clear_of_the_stop_threshold_and_stop_where_they_should():
    for C in (1, 2, 3):
        c = R.infer_case(C)
        f = R.infer_frame_reference(c)
        dropped = int((~f["keep"]).sum())
        print(f"C = {C}: {dropped} of {c['N']} rays come within the bar of the stop threshold")
        assert dropped <= c["N"] // 100
        used = {(n, p): int(f["used"][int(c["rays"][k, 0])]) for k, (n, p) in enumerate(c["spec"]) if p != "gradual"}
        assert used[(40, 2)] == 4 and used[(40, 6)] == 8 and used[(40, 7)] == 9      # first group, a group's edge, the next's start
        assert used[(24, 22)] == 24 and used[(24, 23)] == 24 and used[(40, None)] == 40


def test_the_c_oracle_passes_the_inference_bars():
    """Two rounds of composite_rays (8 and 16 samples a ray): the second on the survivors, from the first one's fp32 sums."""
    from oracle import oracle as O
    c = R.infer_case(3)
    N = c["N"]
    W = R.Worst()
    ws, depth, image = np.zeros(N, R.F32), np.zeros(N, R.F32), np.zeros((N, 3), R.F32)
    alive = list(range(N))
    rays_t = c["nears"][c["rays"][:, 0]].copy()
    ended = []
    for rnd in (0, 1):
        ids = c["rays"][alive, 0]
        ref, keep = R.infer_round_reference(c, rnd, alive, rays_t, ws, depth, image)
        sig, dl, rgb = R.infer_round_inputs(c, rnd, alive)
        O.composite_rays(len(alive), R.INFER_STEPS[rnd], ids.astype(np.int32), rays_t, sig, rgb, dl, ws, depth, image)
        assert keep.mean() >= 0.99
        for name, got in (("rays_t", rays_t), ("ws", ws[ids]), ("depth", depth[ids]), ("image", image[ids])):
            r = ref["t" if name == "rays_t" else name]
            W.compare(f"oracle composite_rays round {rnd}", f"{name} round {rnd}", (r[0][keep], r[1][keep]), got[keep],
                      np.full(int(keep.sum()), "INFER", dtype=object))
        ended.append(int((rays_t < 0).sum()))
        alive = [n for n, t in zip(alive, rays_t) if t >= 0]
        rays_t = rays_t[rays_t >= 0].copy()
    print(W.report(f"C oracle, composite_rays; rays ended per round: {ended}, alive after both: {len(alive)}"))
    assert not W.fails, "\n".join(W.fails)
    assert ended[0] > 10 and ended[1] > 10 and len(alive) > 5
