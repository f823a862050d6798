"""Which torch calls still launch a kernel of their own inside one training step?  bench.py's headline configuration (EquiUnet-48,
2 patches, bf16 autocast, fused Dice, Ranger2020); seven warm steps (optimizer state, the first look-ahead sync), then one step
with (a) the Python-level torch calls that can launch something logged with their call site in brats21_amd, (b) torch.profiler's
list of the aten ops that did launch a kernel or a copy, in order, and (c) the native kernels / copies counted by name.

    python scripts/native_launches.py [PATCH = 128]          (profiles/loss_end_native_launches.txt)
"""
import argparse
import collections
import contextlib
import io
import sys
import traceback

import torch

sys.path.insert(0, ".")
from brats21_amd import get_model, synth  # noqa: E402
from brats21_amd.engine import TrainStep  # noqa: E402
from brats21_amd.optim import Ranger2020  # noqa: E402

patch = int(sys.argv[1]) if len(sys.argv) > 1 else 128
dev = torch.device("cuda:0")
ns = argparse.Namespace(model="equiunet", width=48, norm="group", act="relu", num_classes=3, dropout=0)
with contextlib.redirect_stdout(io.StringIO()):
    m = get_model(ns).to(dev).train()
    opt = Ranger2020(m.parameters(), lr=1e-4, alpha=0.5, k=6, N_sma_threshhold=5, betas=(.95, 0.999), eps=1e-5, weight_decay=1e-5)
step = TrainStep(m, opt, criterion=None, amp=True, amp_dtype=torch.bfloat16)
x, t = synth.random_image(2, 4, (patch,) * 3, seed=1, device=dev), synth.nested_spheres(2, (patch,) * 3, device=dev)
for _ in range(7):
    step(x, t)
torch.cuda.synchronize()

LOG = collections.Counter()
ON = [False]


def site():
    fr = [f for f in traceback.extract_stack()[:-2] if "brats21_amd" in f.filename]
    return " <- ".join(f"{f.filename.split('brats21_amd/')[-1]}:{f.lineno}" for f in fr[-3:][::-1])


def wrap(owner, name, cond=None):
    orig = getattr(owner, name)

    def w(*a, **k):
        if ON[0]:
            try:
                ok = cond(*a, **k) if cond else True
            except Exception:
                ok = True
            if ok:
                first = a[0] if a else None
                if isinstance(first, torch.Tensor):
                    shape = tuple(first.shape)
                elif isinstance(first, (tuple, list)) and any(isinstance(v, torch.Tensor) for v in first):
                    shape = [tuple(v.shape) for v in first]  # (never str() of a tensor: that launches kernels of its own)
                else:
                    shape = first
                LOG[(f"{getattr(owner, '__name__', owner)}.{name}", str(shape)[:40], site())] += 1
        return orig(*a, **k)
    setattr(owner, name, w)


def is_cuda(*a, **k):
    return any(isinstance(v, torch.Tensor) and v.is_cuda for v in a)


def dev_kw(*a, **k):
    return "cuda" in str(k.get("device", ""))


for n in ("zeros", "ones", "full"):
    wrap(torch, n, dev_kw)
for n in ("zeros_like", "ones_like", "full_like", "stack", "cat", "where"):
    wrap(torch, n)
T = torch.Tensor
for n in ("zero_", "fill_", "copy_", "clone", "to", "sum", "mean", "__setitem__", "__add__", "__radd__", "__iadd__", "__mul__", "__rmul__",
          "__imul__", "__sub__", "__rsub__", "__truediv__", "__rtruediv__", "__pow__", "add", "add_", "mul", "mul_", "div"):
    wrap(T, n, is_cuda)
wrap(T, "contiguous", lambda s, *a, **k: s.is_cuda and not s.is_contiguous())
wrap(T, "float", lambda s, *a, **k: s.is_cuda and s.dtype != torch.float32)

from torch.profiler import ProfilerActivity, profile  # noqa: E402
ON[0] = True
with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
    step(x, t)
    torch.cuda.synchronize()
ON[0] = False
print("==== python-level torch calls in one step (count, call, first argument's shape, call site)")
for (op, shape, where), c in sorted(LOG.items(), key=lambda kv: -kv[1]):
    print(f"{c:4d} {op:22s} {shape:40s} {where}")
print("==== aten ops that launched a kernel or a copy in the step, in order")
for e in sorted(prof.events(), key=lambda e: e.time_range.start):
    ks = getattr(e, "kernels", None) or []
    if e.name.startswith("aten::") and ks:
        print(f"  {e.name:24s} thread {e.thread} {[k.name[:60] for k in ks]}")
kern = collections.Counter()
for e in prof.events():
    if str(getattr(e, "device_type", "")).endswith("CUDA") and any(s in e.name for s in ("at::native", "Memcpy", "Memset", "copyBuffer", "fillBuffer")):
        kern[e.name[:110]] += 1
print("==== native device kernels / copies of the step")
for k, c in sorted(kern.items(), key=lambda kv: -kv[1]):
    print(f"{c:4d} {k}")
