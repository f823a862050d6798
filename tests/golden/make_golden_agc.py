"""Generates tests/golden/agc.npz from the REFERENCE's own AGC class (learning/lr_scheduler.py:133-241, imported under
oracle/refshim.py; the module needs only torch) and from torch.nn.utils.clip_grad_norm_, both in float32 on the CPU.

Run here only (the GPU box has no reference checkout):  python tests/golden/make_golden_agc.py

AGC wraps torch.optim.SGD(lr=0): the parameters do not move and p.grad after step() IS the clipped gradient.  ``params`` is
passed as a list (a generator would be exhausted by the first step, see brats21_amd.optim.AGC).

Parameters (PARAMS below): the smallest shapes on which each path of csrc/gradclip.hip can go wrong -- contiguous units
whose length is / is not a multiple of 4, a unit of 8100 elements, tensors of more than one 2048-element chunk with a ragged
tail, strided column units, one-element units, 1-D and one-element tensors, an EvoNorm-style (1,C,1,1,1) tensor, an all-zero
parameter (the eps branch), a unit whose gradient is zero, a parameter without a gradient.  Unit norms of the parameters
alternate between ~0.015 and ~1 so that case (b) has both outcomes in every tensor.

Cases:
  a  AGC, defaults (clipping 1e-2, eps 1e-3); gradients scaled PER UNIT to grad_norm / max_norm in [1.5, 4] or [0.2, 0.6]
     (plain randn * 0.01 gradients trigger nearly everywhere)
  b  AGC, clipping 1e-5, unit gradient norms of about 5e-7: triggered units go through max(grad_norm, 1e-6)
  c  clip_grad_norm_ on a's gradients with max_norm = half their norm        d  ... with max_norm = twice their norm (no clip)
  e  clip_grad_norm_ (coefficient ~0.5) then AGC with the defaults on twice a's gradients (the step's order)
Before writing, the script asserts on the reference's numbers: in every multi-unit tensor at least a quarter of the units
trigger and at least a quarter do not (cases a, b, e); every unit's grad_norm / max_norm lies outside [0.95, 1.05]; the
reference's f32 result is within rtol 1e-5 of the float64 restatement tests/_agc_ref.py.

Arrays only.  `<case>__out<i>` is the reference's f32 gradient of parameter i, `<case>__out<i>__f64` the float64 result of
tests/_agc_ref.py rounded to f32 once (the value the GPU test compares with); for c / d, whose result is g * clip_coef, the
float64 side is the two scalars `__total_norm__f64` and `__clip_coef__f64`.  Case d's output equals its input (asserted)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import refshim  # noqa: E402

refshim.install()
from learning.lr_scheduler import AGC, unitwise_norm  # noqa: E402
import _agc_ref as R  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
# (shape, zero-valued parameter, has a gradient)
PARAMS = [((5, 24, 3, 3, 3), False, True), ((3, 30, 3, 3, 3), False, True), ((3, 25, 3, 3, 3), False, True),
          ((2, 300, 3, 3, 3), False, True), ((6, 10), False, True), ((1, 8, 1), False, True), ((7,), False, True),
          ((1,), False, True), ((1, 16, 1, 1, 1), False, True), ((4,), True, True), ((3, 5), False, False)]
ZERO_GRAD_UNIT = (0, 0)  # (parameter, unit): this unit's gradient is zero in every case
RTOL = 1e-5


def per_unit(x, unit_values):
    """Scale every unit of x (unitwise_norm's units) to the norm given for it."""
    n = unitwise_norm(x.double())
    v = torch.as_tensor(unit_values, dtype=torch.float64).reshape(n.shape)
    return (x.double() * (v / n)).float()


def nunits(shape):
    return int(unitwise_norm(torch.ones(shape)).numel())


def make_params(gen):
    ps = []
    for shape, zero, _ in PARAMS:
        if zero:
            ps.append(torch.zeros(shape))
            continue
        n = nunits(shape)
        small = torch.arange(n) % 2 == (0 if n > 1 else len(ps) % 2)  # unit norm ~0.015, the others ~1
        norms = torch.where(small, 0.01 + 0.01 * torch.rand(n, generator=gen), 0.2 + 1.8 * torch.rand(n, generator=gen))
        ps.append(per_unit(torch.randn(shape, generator=gen), norms))
    return ps


def grads_by_ratio(gen, params, clipping, eps):
    """Unit u of a multi-unit tensor triggers when u % 4 is 1 or 2; single-unit tensors alternate."""
    gs = []
    for i, (p, (shape, _, has)) in enumerate(zip(params, PARAMS)):
        if not has:
            gs.append(None)
            continue
        n = nunits(shape)
        trig = ((torch.arange(n) % 4 == 1) | (torch.arange(n) % 4 == 2)) if n > 1 else torch.tensor([i % 2 == 0])
        ratio = torch.where(trig, 1.5 + 2.5 * torch.rand(n, generator=gen), 0.2 + 0.4 * torch.rand(n, generator=gen))
        mx = torch.clamp(unitwise_norm(p.double()), min=eps).reshape(-1) * clipping
        gs.append(per_unit(torch.randn(shape, generator=gen), ratio.double() * mx))
    return gs


def grads_by_norm(gen, lo, hi):
    gs = []
    for shape, _, has in PARAMS:
        n = nunits(shape)
        gs.append(per_unit(torch.randn(shape, generator=gen), lo + (hi - lo) * torch.rand(n, generator=gen)) if has else None)
    return gs


def zero_unit(gs):
    i, u = ZERO_GRAD_UNIT
    gs[i][u] = 0.0
    return gs


def run_reference(params, grads, max_norm, agc_kw):
    """-> (clipped gradients f32, total_norm f32 or None), from the reference's AGC / torch's clip_grad_norm_."""
    ps = [torch.nn.Parameter(p.clone()) for p in params]
    for p, g in zip(ps, grads):
        p.grad = None if g is None else g.clone()
    total = None
    if max_norm is not None:
        total = torch.nn.utils.clip_grad_norm_(ps, max_norm)
    if agc_kw is not None:
        opt = AGC(list(ps), torch.optim.SGD(ps, lr=0.0), **agc_kw)
        opt.step()
    assert all(torch.equal(p.detach(), q) for p, q in zip(ps, params))
    return [p.grad for p in ps], total


def main():
    gen = torch.Generator().manual_seed(20211018)
    params = make_params(gen)
    ga = zero_unit(grads_by_ratio(gen, params, 1e-2, 1e-3))
    gb = zero_unit(grads_by_norm(gen, 3e-7, 8e-7))
    ge = [None if g is None else g * 2.0 for g in ga]
    norm_a = float(torch.sqrt(sum((g.double() ** 2).sum() for g in ga if g is not None)))
    cases = {  # name: (gradients, max_norm, AGC keywords)
        "a": (ga, None, dict(clipping=1e-2, eps=1e-3)),
        "b": (gb, None, dict(clipping=1e-5, eps=1e-3)),
        "c": (ga, 0.5 * norm_a, None),
        "d": (ga, 2.0 * norm_a, None),
        "e": (ge, norm_a, dict(clipping=1e-2, eps=1e-3)),
    }
    arrays = {"shapes": np.array([str(tuple(s)) for s, _, _ in PARAMS]), "has_grad": np.array([h for _, _, h in PARAMS]),
              "zero_grad_unit": np.array(ZERO_GRAD_UNIT, np.int64), "cases": np.array(list(cases))}
    for i, p in enumerate(params):
        arrays[f"param{i}"] = p.numpy()
    for name, gs in (("a", ga), ("b", gb)):  # c, d use a's; e uses 2 * a's
        for i, g in enumerate(gs):
            if g is not None:
                arrays[f"grad_{name}{i}"] = g.numpy()
    arrays["grad_source"] = np.array(["a", "b", "a", "a", "2a"])
    live = [i for i, (_, _, h) in enumerate(PARAMS) if h]
    for name, (gs, max_norm, agc_kw) in cases.items():
        out, total = run_reference(params, gs, max_norm, agc_kw)
        assert out[-1] is None and PARAMS[-1][2] is False
        g64, total64, coef64, trig, ratio = R.clip_then_agc([params[i] for i in live], [gs[i] for i in live], max_norm,
                                                             agc_kw and agc_kw["clipping"], agc_kw["eps"] if agc_kw else 0.0)
        arrays[f"{name}__max_norm"] = np.array(-1.0 if max_norm is None else max_norm, np.float64)
        arrays[f"{name}__clipping"] = np.array(-1.0 if agc_kw is None else agc_kw["clipping"], np.float64)
        arrays[f"{name}__eps"] = np.array(-1.0 if agc_kw is None else agc_kw["eps"], np.float64)
        if total is not None:
            arrays[f"{name}__total_norm"] = total.numpy()
            arrays[f"{name}__total_norm__f64"] = total64.numpy()
            arrays[f"{name}__clip_coef__f64"] = coef64.numpy()
            assert abs(float(total) - float(total64)) <= RTOL * float(total64)
            assert (float(coef64) < 1.0) == (name != "d"), (name, float(coef64))
        worst = 0.0
        for k, i in enumerate(live):
            ref, f64 = out[i], g64[k].float()
            err = float(((ref.double() - f64.double()).abs() / f64.double().abs().clamp_min(1e-300)).max())
            worst = max(worst, err)
            assert torch.allclose(ref, f64, rtol=RTOL, atol=0.0), (name, i, err)
            if name == "d":
                assert torch.equal(ref, gs[i])
                continue
            arrays[f"{name}__out{i}"] = ref.numpy()
            if agc_kw is not None:
                arrays[f"{name}__out{i}__f64"] = f64.numpy()
        ntrig = 0
        for k, i in enumerate(live):
            if agc_kw is None:
                break
            t, r = trig[k], ratio[k]
            assert not bool(((r >= 0.95) & (r <= 1.05)).any()), (name, i, r)
            if t.numel() > 1:
                assert 4 * int(t.sum()) >= t.numel() and 4 * int((~t).sum()) >= t.numel(), (name, i, t)
            ntrig += int(t.sum())
        if agc_kw is not None:
            i, u = ZERO_GRAD_UNIT
            assert not bool(trig[live.index(i)][u]) and float(out[i][u].abs().max()) == 0.0
        print(f"case {name}: worst rel err of the reference's f32 result vs float64 {worst:.2e}; units triggered {ntrig}"
              + (f"; total_norm {float(total):.6g} coef {float(coef64):.6g}" if total is not None else ""))
    # case b reaches max(grad_norm, 1e-6): triggered units with a gradient norm below 1e-6 exist
    _, _, _, trig, _ = R.clip_then_agc([params[i] for i in live], [gb[i] for i in live], None, 1e-5, 1e-3)
    below = sum(int((t & (unitwise_norm(gb[i].double()).reshape(-1) < 1e-6)).sum()) for t, i in zip(trig, live))
    assert below > 10, below
    path = os.path.join(OUT, "agc.npz")
    np.savez_compressed(path, **arrays)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
