"""Library call trace of the network programs, the stand-alone blocks and the criteria: for each network configuration, every libbrats_hip entry-point call of two training
steps (engine.TrainStep, deep supervision on; the second step is the one that runs on a pack plan / DDP bucket slices) and of
two no_grad eval forwards (the second one hits the packed-weight and BCNorm fold caches), followed by a sha256 of the losses,
every parameter gradient and the eval logits (the U-Net family: also a backward of a loss on the deep heads only and one of a loss
on d1 only); for a block (networks.RRCNNblock, networks.CBAM, networks.AttentionBlock) one forward + backward, for a
criterion of losses.py one loss + gradient at 32^3.  A call is written as its name, its arguments -- pointers as 0 (null) or 1,
integers and floats verbatim; kinds from _lib._parse_header() -- and its return value.  Two trees compute the same thing the same
way when their outputs are identical:

    python scripts/call_trace.py OUT.txt [--tree OTHER_CHECKOUT] [--only REGEX] [--no-full]
    python scripts/call_trace.py OUT.txt --digest        (no GPU: lines and sha256 per configuration of an existing OUT.txt, the
                                                           form small enough to commit under profiles/)
"""
import argparse, contextlib, hashlib, io, re, sys, warnings

ap = argparse.ArgumentParser()
ap.add_argument("out")
ap.add_argument("--tree", default=".", help="the checkout whose brats21_amd is traced")
ap.add_argument("--only", default=None, help="run the configurations whose name matches")
ap.add_argument("--no-full", action="store_true", help="skip the 128^3 cases")
ap.add_argument("--digest", action="store_true", help="print the per-configuration digest of the existing output file")
args = ap.parse_args()
if args.digest:
    txt = open(args.out).read()
    print(f"whole file: {txt.count(chr(10))} lines sha256 {hashlib.sha256(txt.encode()).hexdigest()}")
    for sec in txt.split("==== ")[1:]:
        print(f"{sec.split(chr(10), 1)[0]}: {sec.count(chr(10))} lines sha256 {hashlib.sha256(sec.encode()).hexdigest()}")
    sys.exit(0)
sys.path.insert(0, args.tree)

import torch
from brats21_amd import _lib, get_model, synth
from brats21_amd.ddp import GradientBuckets
from brats21_amd.engine import TrainStep
from brats21_amd.optim import Ranger2020

LOG = []


class _Recorder:
    """Stands in for the loaded library (_lib._lib): every entry point is called through, and logged."""

    def __init__(self, real):
        self._real, self._sigs = real, _lib._parse_header()

    def __getattr__(self, name):
        fn, (_, spec) = getattr(self._real, name), self._sigs[name]

        def call(*a):
            ret = fn(*a)
            shown = [("0" if v is None or v == 0 else "1") if k == "p" else repr(v) for k, v in zip(spec, a)]
            LOG.append(f"{name}({', '.join(shown)}) -> {ret!r}")
            return ret
        setattr(self, name, call)
        return call


def sha(t):
    return hashlib.sha256(t.detach().float().cpu().contiguous().numpy().tobytes()).hexdigest()


def flat(o):
    """The tensors of a (nested) tuple / list of outputs, in order."""
    return [o] if torch.is_tensor(o) else [t for e in o for t in flat(e)]


def run(name, model, width, size=32, precision="bf16", norm="group", act="relu", dropout=0, buckets=False, num_classes=3,
        deep_supervision=True, t=2, heads=False, **attrs):
    """model "unet" / "r2unet": networks.Unet / R2Unet built directly (num_classes, deep_supervision, t are theirs alone).  heads:
    two more backwards follow the training steps, one of a loss on the deep heads only and one of a loss on d1 only."""
    if args.only and not re.search(args.only, name):
        return
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    ns = argparse.Namespace(model=model, width=width, norm=norm, act=act, num_classes=3, dropout=dropout)
    feats = [width * 2 ** i for i in range(4)]
    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if model == "att_equiunet":  # (not in the factory: built like the factory builds EquiUnet)
            from brats21_amd.networks import AttEquiUnet
            m = AttEquiUnet(4, 3, feats, norm, act, deep_supervision=True, dropout=dropout).to(dev).train()
        elif model == "unet":
            from brats21_amd.networks import Unet
            m = Unet(4, num_classes, feats, norm, act, deep_supervision=deep_supervision).to(dev).train()
        elif model == "r2unet":  # (not in the factory)
            from brats21_amd.networks import R2Unet
            m = R2Unet(4, num_classes, feats, t, norm, act, deep_supervision=deep_supervision).to(dev).train()
        else:
            m = get_model(ns).to(dev).train()
    m.precision = precision
    for k, v in attrs.items():
        assert hasattr(m, k), k
        setattr(m, k, v)
    opt = Ranger2020(m.parameters(), lr=1e-4, weight_decay=1e-5, use_gc=False)
    step = TrainStep(m, opt, amp=False, buckets=GradientBuckets(m) if buckets else None)
    x, tgt = synth.random_image(2, 4, (size,) * 3, seed=1, device=dev), synth.nested_spheres(2, (size,) * 3, device=dev)
    tgt = tgt[:, [c % 3 for c in range(num_classes)]].contiguous()  # (three spheres: repeated for more classes)

    def grads():
        return [f"grad {k} {sha(p.grad) if p.grad is not None else None}" for k, p in m.named_parameters()]

    out = [f"==== {name}"]
    for i in (1, 2):
        del LOG[:]
        loss = step(x, tgt)
        out += [f"-- train step {i}"] + LOG[:] + [f"loss {sha(loss)}"]
    out += grads()
    if heads:
        # (autograd hands a Function zeros for the heads the loss does not use, not None: these backwards run every head's pass on a
        #  zero gradient; the programs' `dout is None` branches are reached only by a caller that bypasses autograd)
        for label, pick in (("the deep heads only", slice(1, None)), ("d1 only", slice(0, 1))):
            m.zero_grad(set_to_none=True)
            del LOG[:]
            picked = flat(m(x))[pick]
            if picked:
                loss = sum(o.float().square().mean() for o in picked)
                loss.backward()
                out += [f"-- forward + backward of a loss on {label}"] + LOG[:] + [f"loss {sha(loss)}"] + grads()
    m.eval()
    for i in (1, 2):
        del LOG[:]
        with torch.no_grad():
            logits = m(x)
        out += [f"-- eval forward {i}"] + LOG[:]
        out += [f"logits {sha(o)}" for o in flat(logits)]
    torch.cuda.synchronize()
    with open(args.out, "a") as f:
        f.write("\n".join(out) + "\n")
    print(f"{name}: {len(out)} lines", flush=True)


def traced(name, fn):
    """One stand-alone piece: fn() -> tensors to hash; its calls and hashes go to the output like a network's."""
    if args.only and not re.search(args.only, name):
        return
    torch.manual_seed(0)
    del LOG[:]
    res = fn()
    torch.cuda.synchronize()
    out = [f"==== {name}"] + LOG[:] + [f"result {i} {sha(t) if t is not None else None}" for i, t in enumerate(res)]
    with open(args.out, "a") as f:
        f.write("\n".join(out) + "\n")
    print(f"{name}: {len(out)} lines", flush=True)


def block(make, cin, size=16, gated=False):
    """forward + backward of an nn.Module block on an NCDHW input (gated: on a gating signal g and the input, AttentionBlock's
    forward(g, x)): -> (output, input gradient(s), parameter gradients)."""
    dev = torch.device("cuda:0")
    m = make().to(dev).train()
    xs = [synth.random_image(2, cin, (size,) * 3, seed=s, device=dev).requires_grad_(True) for s in ((2, 1) if gated else (1,))]
    y = m(*xs)
    y.backward(torch.ones_like(y) / y.numel())
    return [y] + [x.grad for x in xs] + [p.grad for p in m.parameters()]


def criterion(make, boundary=False, labels=False):
    from brats21_amd import transforms
    dev = torch.device("cuda:0")
    t = synth.nested_spheres(2, (32,) * 3, device=dev)
    x = (synth.random_image(2, 3, (32,) * 3, seed=2, device=dev) * 3).requires_grad_(True)
    target = [t, transforms.one_hot_to_dist(t)] if boundary else (t.sum(1, keepdim=True) if labels else t)
    loss = make()(x, target)
    loss.backward()
    return [loss, x.grad]


_lib._lib = _Recorder(_lib.lib())
open(args.out, "w").close()
for net in ("equiunet", "equiunet_assp_evo"):
    for prec in ("bf16", "fp16", "fp32", "x3", "bf16x3"):
        run(f"{net}-16-{prec}", net, 16, precision=prec)
    for plan in (True, False):
        run(f"{net}-16-bf16-pack_plan={plan}", net, 16, pack_plan=plan)
    run(f"{net}-16-bf16-dropout", net, 16, dropout=0.1)
    for fold in ("fold_head_bwd", "fold_pool_bwd", "fold_bwd_stats", "fold_head_fwd"):
        run(f"{net}-16-bf16-{fold}=False", net, 16, **{fold: False})
    for fp8 in ("fwd", "all"):
        run(f"{net}-48-bf16-fp8={fp8}", net, 48, conv_fp8=fp8)
    run(f"{net}-48-bf16-buckets", net, 48, buckets=True)
for norm in ("group", "instance", "batch", "bcn"):
    for act in ("relu", "leakyrelu", "prelu"):
        if (norm, act) != ("batch", "prelu"):  # (not implemented: EquiUnet.__init__)
            run(f"equiunet-8-fp32-{norm}-{act}", "equiunet", 8, precision="fp32", norm=norm, act=act)
run("equiunet-16-bf16-norm_on_load=False", "equiunet", 16, norm_on_load=False)
if not args.no_full:  # the only shape that takes the 256 MiB affine_act_pool branch
    run("equiunet-48-bf16-128", "equiunet", 48, size=128)
for prec in ("bf16", "fp32"):
    run(f"modified_unet-16-{prec}", "modified_unet", 16, precision=prec)
    run(f"att_equiunet-16-{prec}", "att_equiunet", 16, precision=prec, norm="instance")
    run(f"equiunet_ref-16-{prec}", "equiunet_ref", 16, precision=prec)
# the U-Net family (networks/unet.py, networks/r2unet.py), with the backwards of partial losses
for prec in ("bf16", "fp16", "fp32", "x3"):
    run(f"unet-16-{prec}", "unet", 16, precision=prec, heads=True)
run("unet-16-bf16-instance-leakyrelu", "unet", 16, norm="instance", act="leakyrelu", heads=True)
for switch in ("fold_head_bwd", "fold_head_fwd", "fold_pool_bwd", "fold_bwd_stats", "norm_on_load"):
    run(f"unet-16-bf16-{switch}=False", "unet", 16, heads=True, **{switch: False})
run("unet-16-bf16-num_classes=5", "unet", 16, num_classes=5, heads=True)  # (the head fold is not taken)
run("unet-16-bf16-deep_supervision=False", "unet", 16, deep_supervision=False, heads=True)
run("unet-16-bf16-skip_deep_heads_in_eval", "unet", 16, heads=True, skip_deep_heads_in_eval=True)
for prec in ("bf16", "fp16", "fp32"):
    run(f"r2unet-16-{prec}", "r2unet", 16, precision=prec, heads=True)
for t in (1, 3):
    run(f"r2unet-16-bf16-t={t}", "r2unet", 16, t=t, heads=True)
run("r2unet-16-bf16-instance", "r2unet", 16, norm="instance", heads=True)
run("r2unet-16-bf16-deep_supervision=False", "r2unet", 16, deep_supervision=False, heads=True)
if not args.no_full:  # the only shapes that take the 256 MiB one-pass pool branches
    run("unet-48-bf16-128", "unet", 48, size=128)
    run("r2unet-48-bf16-128", "r2unet", 48, size=128)
from brats21_amd import losses
from brats21_amd.networks import CBAM, AttentionBlock, RRCNNblock
for norm, act in (("group", "relu"), ("instance", "leakyrelu")):
    traced(f"RRCNNblock-{norm}-{act}", lambda: block(lambda: RRCNNblock(8, 16, norm, act, 2), 8))
traced("CBAM-16", lambda: block(lambda: CBAM(16), 16))
traced("AttentionBlock-16-16-8", lambda: block(lambda: AttentionBlock(16, 16, 8), 16, gated=True))
_IDC, _SIG = [0, 1, 2], dict(include_background=True, sigmoid=True, softmax=False, squared_pred=True, reduction="mean")
for name, make, kw in (
        ("dice", lambda: losses.DiceLoss(), {}), ("jaccard", lambda: losses.DiceLoss(jaccard=True), {}),
        ("hd", lambda: losses.HausdorffLoss(_IDC, alpha=2, sigmoid=True), {}),
        ("boundary", lambda: losses.BoundaryLoss(_IDC, sigmoid=True), dict(boundary=True)),
        ("dice_hd", lambda: losses.DiceHDLoss(idc_hd=_IDC, alpha_hd=2, hybrid=False, weight_hd=0.5, weight_dice=0.5, **_SIG), {}),
        ("dice_boundary", lambda: losses.DiceBoundaryLoss(idc_boundary=_IDC, **_SIG), dict(boundary=True)),
        ("softmax_dice_ce", lambda: losses.SoftmaxDiceCELoss(), dict(labels=True)),
        ("dice_ce", lambda: losses.DiceCELoss(batch=True, **_SIG), {}), ("dice_focal", lambda: losses.DiceFocalLoss(batch=False, **_SIG), {}),
        ("focal", lambda: losses.FocalLoss(gamma=2.0, reduction="mean"), {}),
        ("tversky", lambda: losses.TverskyLoss(include_background=True, sigmoid=True, softmax=False, alpha=0.5, beta=0.5, reduction="mean"), {})):
    traced(f"criterion-{name}", lambda: criterion(make, **kw))
