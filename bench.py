#!/usr/bin/env python3
"""bench.py -- BASELINE.json's metric on MI355X: train patches/s of EquiUnet width 48 on synthetic
4x128^3 patches, batch 2 per GPU, bf16 (configs[1]); one "step" = forward + deep-supervision Dice
loss + backward + gradient all-reduce (N > 1) + fused Ranger2020 step (the reference's default optimizer; --optimizer adam for
torch's Adam).  Prints ONE JSON line on rank 0.

A plain run sets up, warms up, times the steps, writes the last step's outputs (--dump-outputs DIR) and prints the line.  With
--full the line also carries everything else, measured AFTER the headline's timed region: the box probe, the dominant kernel's
roofline (per-kernel HIP events in two of the timed steps) and live HBM traffic, the host-enqueue time and `ddp` accounting, at
N = 1 the other stated configurations as short legs (configs2_per_gpu, configs4_per_gpu, fp16_mode, inference*, parity_mode) and
the CPU baseline, at N > 1 the graph leg (graph_ddp).

  python bench.py --gpus 1 --steps 5 --warmup 2 [--dump-outputs DIR] [--full]
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \\
         bench.py --gpus N --steps K --warmup W
"""
import argparse
import json
import os
import sys
import time

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

KFD_NODES = "/sys/class/kfd/kfd/topology/nodes"   # (module-level so that tests can point them at a fake tree)
PCI_DEVICES = "/sys/bus/pci/devices"
PEAK_BF16_TFLOPS = 2500.0   # dense bf16 MFMA, MI355X_MICROARCH.md
PEAK_F32_TFLOPS = 157.3
PEAK_FP8_TFLOPS = 5000.0    # dense MX-scaled e4m3 MFMA (--fp8 only)


def conv_flops(cin, cout, k, n, d, h, w):
    return 2.0 * cin * k ** 3 * cout * n * d * h * w


DUMP_BUDGET_BYTES = 48 << 20  # parameters + gradients together; the loss adds 4 bytes (cap: 64 MB)


def dump_outputs(out_dir, loss, model):
    """--dump-outputs DIR: what the last timed step handed its caller, as float32 .npy files -- loss.npy (the step's return
    value) and, per parameter of the model it updated, param.<name>.npy (the weights after the optimizer step) and
    grad.<name>.npy (the step's gradient).  A tensor larger than the per-tensor share of DUMP_BUDGET_BYTES is reduced to a
    fixed sample: flat indices drawn from a CPU generator seeded with the parameter's position, sorted -- the same elements in
    every run of the same configuration, so two builds compare output for output."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "loss.npy"), loss.detach().float().cpu().numpy())
    params = list(model.named_parameters())
    per_tensor = DUMP_BUDGET_BYTES // (2 * 4 * len(params))
    for i, (name, p) in enumerate(params):
        idx = None
        if p.numel() > per_tensor:
            g = torch.Generator().manual_seed(i)
            idx = torch.randint(p.numel(), (per_tensor,), generator=g).sort().values.to(p.device)
        for kind, v in (("param", p), ("grad", p.grad)):
            if v is None:
                continue
            flat = v.detach().reshape(-1)
            np.save(os.path.join(out_dir, f"{kind}.{name}.npy"), (flat if idx is None else flat[idx]).float().cpu().numpy())


def cpu_baseline(width, cores):
    """The CPU oracle (plain torch fp32 restatement of the reference's CPU path, oracle/unet.py) timed on the GPU box's
    host cores on a bounded sample of the bench workload: ONE real 4x128^3 patch of the width-48 network, forward + Dice
    loss + backward, 3 warm-ups + 5 timed repetitions, MEDIAN (>= 3 warm-ups + >= 5 timed; the
    counts are also machine-readable fields of the record).  Reported in the metric's unit
    (128^3-patches/s).  Threads: torch/mkldnn 3D convolutions scale to ~16 threads on this host and get SLOWER beyond
    (measured on the GPU box, scripts/cpu_threads.py: 8 thr 0.14 s, 16 thr 0.10 s, 32 thr 0.15 s, 64 thr 0.43 s, 128 thr
    2.1 s per 32^3 patch), so the baseline uses min(16, cores) threads."""
    from oracle import synth as osynth, unet
    threads = min(16, cores)
    torch.set_num_threads(threads)
    sd = {k: v.requires_grad_(True) for k, v in osynth.fill_state_dict(unet.equiunet_state_shapes(width)).items()}

    def run(size, warm, timed):
        x, t = osynth.random_image(1, 4, size), osynth.nested_spheres(1, size)
        times = []
        for it in range(warm + timed):
            t0 = time.perf_counter()
            loss = unet.deep_supervision_loss(unet.equiunet_forward(sd, x), t)
            loss.backward()
            for v in sd.values():
                v.grad = None
            if it >= warm:
                times.append(time.perf_counter() - t0)
        return times

    warm, timed = 3, 5
    t128 = sorted(run((128, 128, 128), warm, timed))
    med = t128[timed // 2]
    return {"value": round(1.0 / med, 5), "unit": "patches/s", "cores": threads, "kind": "port", "warmup_reps": warm, "timed_reps": timed,
            "sample": f"1 patch of 4x128^3, fwd+Dice+bwd fp32 torch CPU (oracle/unet.py), {warm} warm-ups + {timed} timed, median {med:.2f} s "
                      f"(min {t128[0]:.2f}, max {t128[-1]:.2f}); host has {cores} cores, {threads} threads used (fastest setting)"}


def parity_mode_leg(args, dev, x, t):
    """The 1e-3-logit-parity configurations of the SAME workload, 4 warm-up + 8 timed training steps (exact f32: 2 + 4), plus the logit
    error of each mode against the CPU oracle on one patch of the bench's own image with the bench's own initial weights
    (the oracle is only the checker here):
      * model.precision = "x3": f32 tensors, the 3x3x3 convolutions as three fp16-pair MFMA products with f32 accumulation
        (csrc/conv_igemm_x3.hpp; dY scaled from its recorded |max| in the backward) -- the reported parity mode;
      * model.precision = "fp32": the exact-f32 MFMA kernels (v_mfma_f32_16x16x4_f32), kept beside it as "fp32_exact"."""
    import argparse as _ap, contextlib, io
    from brats21_amd import get_model
    from brats21_amd.engine import TrainStep
    from brats21_amd.optim import Ranger2020
    from oracle import unet
    torch.manual_seed(0)
    ns = _ap.Namespace(model=args.model, width=args.width, norm="group", act="relu", num_classes=3, dropout=0)
    with contextlib.redirect_stdout(io.StringIO()):
        m = get_model(ns)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m = m.to(dev)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    fwd = unet.equiunet_forward if args.model == "equiunet" else unet.assp_evo_forward
    with torch.no_grad():
        ref = fwd(sd, x[:1].float().cpu())[0]
    legs = {}
    for prec in ("x3", "fp32"):
        m.load_state_dict(sd)
        m.precision = prec
        m.eval()
        with torch.no_grad():
            err = float((m(x[:1])[0].float().cpu() - ref).abs().max())
        m.train()
        with contextlib.redirect_stdout(io.StringIO()):
            opt = Ranger2020(m.parameters(), lr=1e-4, alpha=0.5, k=6, N_sma_threshhold=5, betas=(.95, 0.999), eps=1e-5, weight_decay=1e-5)
        step = TrainStep(m, opt, criterion=None, amp=False)
        nw, nt = (4, 8) if prec == "x3" else (2, 4)  # (x3: a 2 + 5 leg read 0.3 ms high beside 10 + 30, 4 + 8 does not; f32: 145 ms / step)
        for _ in range(nw):
            step(x, t)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(nt):
            step(x, t)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / nt * 1e3
        legs[prec] = {"dtype": prec, "ms_per_step": round(ms, 2), "patches_per_s": round(x.shape[0] / ms * 1e3, 2),
                      "logit_err": float(f"{err:.3e}")}
    out = dict(legs["x3"])
    out.update({"dtype": "x3 (f32 storage; 3x3x3 convolutions = 3 fp16-pair MFMA products, f32 accumulate)", "logit_bar": 1e-3,
                "logit_absmax": round(float(ref.abs().max()), 2), "fp32_exact": legs["fp32"],
                "note": "model.precision='x3' (csrc/conv_igemm_x3.hpp) beside 'fp32' (exact-f32 MFMA): same batch / optimizer, 4 warm-up "
                        "+ 8 timed steps (f32: 2 + 4); logit_err = max abs difference of the main head to the CPU oracle (oracle/unet.py) on "
                        "patch 0 with the initial weights"})
    return out


def side_train_leg(dev, rank, model_name, width, batch, precision, warmup, steps, what, fp8=None, graph=False, patch=128):
    """A short training leg of another stated configuration on a FRESH model (own weights, own optimizer), run after the
    headline's timed region: ``warmup`` untimed + ``steps`` timed steps of the same step body as the headline (forward +
    deep-supervision Dice + backward + fused Ranger2020), fp16 under the reference's GradScaler loop."""
    import argparse as _ap, contextlib, io
    from brats21_amd import get_model, synth
    from brats21_amd.engine import GraphedTrainStep, TrainStep
    from brats21_amd.optim import Ranger2020
    torch.manual_seed(0)
    ns = _ap.Namespace(model=model_name, width=width, norm="group", act="relu", num_classes=3, dropout=0)
    with contextlib.redirect_stdout(io.StringIO()):
        m = get_model(ns).to(dev).train()
        opt = Ranger2020(m.parameters(), lr=1e-4, alpha=0.5, k=6, N_sma_threshhold=5, betas=(.95, 0.999), eps=1e-5, weight_decay=1e-5,
                         capturable=graph or precision == "fp16")  # (fp16: the GradScaler's skip decided on the device, no host round trip)
    if fp8:
        m.conv_fp8 = fp8
    size = (patch,) * 3
    x = synth.random_image(batch, 4, size, seed=1234 + rank, device=dev)
    t = synth.nested_spheres(batch, size, device=dev)
    amp_dtype = torch.float16 if precision == "fp16" else torch.bfloat16
    step = TrainStep(m, opt, criterion=None, amp=True, amp_dtype=amp_dtype)
    if graph:
        step = GraphedTrainStep(step, warmup=2)
    for _ in range(warmup):
        step(x, t)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = step(x, t)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    out = {"config": what, "dtype": precision + (f"+e4m3 conv ({fp8})" if fp8 else ""), "ms_per_step": round(ms, 2),
           "patches_per_s": round(batch / ms * 1e3, 2), "patches_per_gpu": batch, "warmup": warmup, "steps": steps,
           "loss": round(float(loss.item()), 5)}
    if getattr(step, "scaler", None) is not None:
        out["grad_scale"] = float(step.scaler.get_scale())
    del step, opt, m, x, t
    torch.cuda.empty_cache()
    return out


def other_configs_legs(dev, rank, patch=128):
    """The stated configurations the headline line does not time, ~1 s each on one GPU."""
    legs = {}
    legs["configs2_per_gpu"] = side_train_leg(
        dev, rank, "equiunet_assp_evo", 48, 2, "bf16", 5, 10,
        "equiunet_assp_evo width=48, 2 patches of 4x128^3 per GPU, bf16, eager step (BASELINE.json configs[2]: one rank's share of "
        "the 8-GPU batch of 16; the all-reduce is not part of a world-1 leg)", patch=patch)
    legs["configs2_per_gpu"]["as_one_hipgraph"] = side_train_leg(
        dev, rank, "equiunet_assp_evo", 48, 2, "bf16", 3, 10, "the same step replayed as one hipGraph (GraphedTrainStep)", graph=True, patch=patch)
    legs["fp16_mode"] = side_train_leg(
        dev, rank, "equiunet", 48, 2, "fp16", 5, 10,
        "the headline workload (equiunet width=48, 2 x 4x128^3) in the REFERENCE's own arithmetic: torch.autocast(float16) + "
        "GradScaler loop (learning/engine.py:304,117-122), fp16 MFMA kernels; Ranger2020(capturable=True) takes the scaler's loss scale / "
        "overflow flag as device tensors (the _step_supports_amp_scaling protocol): no unscale WRITE pass and no host read per step (the scaler's inf check still reads every gradient once)", patch=patch)
    legs["configs4_per_gpu"] = side_train_leg(
        dev, rank, "equiunet_assp_evo", 64, 4, "fp16", 3, 6,
        "does NOT hold parity (a throughput figure only: e4m3 convolutions move the hard Dice on trained weights by 5e-4 .. 1e-2 against "
        "the CPU oracle, bar 1e-3 -- also when only the 128^3 / 64^3 levels use them; fp16 alone <= 6e-4 everywhere): "
        "equiunet_assp_evo width=64, 4 patches of 4x128^3 per GPU, fp16 storage + e4m3 MFMA convolutions forward / input gradient / "
        "weight gradient (BASELINE.json configs[4]: one rank's share of the 8-GPU batch of 32)", fp8="all", patch=patch)
    legs["configs4_per_gpu"]["holds_parity"] = False
    legs["configs4_per_gpu"]["parity_note"] = (
        "tests/test_trained_gpu.py prints the Dice margins of fp16 + e4m3 (all levels, >= 64^3 only, 128^3 only) beside bf16 / fp16 on "
        "trained weights; profiles/r06_trained_weights_parity.txt.  No restriction of the e4m3 path tried holds the bar on the stress volumes")
    return legs


def gpu_count_without_hip():
    """GPUs this process may use, read from the KFD topology in sysfs and the *_VISIBLE_DEVICES masks -- no HIP / HSA call, so
    the launcher process stays a process that never initialised the GPU (torch.cuda.device_count() may fall through
    to hipGetDeviceCount; ADVICE r5: a device mask narrower than the node must narrow the count).  None = unknown."""
    import glob
    nodes = glob.glob(os.path.join(KFD_NODES, "*", "properties"))
    if not nodes:
        return None
    n = 0
    for p in nodes:
        try:
            props = dict(line.split()[:2] for line in open(p) if len(line.split()) >= 2)
        except PermissionError:
            continue  # a GPU of the node that this container was not given (its KFD node is not readable): not ours to count
        except OSError:
            return None
        if int(props.get("simd_count", "0")) > 0:
            n += 1
    # ROCR_VISIBLE_DEVICES filters what the runtime enumerates, HIP_ / CUDA_VISIBLE_DEVICES what HIP shows of that: each is a
    # comma list of indices (or GPU-<uuid> names); an entry that cannot be an index of the narrower list ends the list
    for var in ("ROCR_VISIBLE_DEVICES", "HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        mask = os.environ.get(var)
        if mask is None:
            continue
        seen = 0
        for item in mask.split(","):
            item = item.strip()
            if item.isdigit():
                if int(item) >= n:
                    break
            elif not item.startswith("GPU-"):
                break
            seen += 1
        n = min(n, seen)
    return n


def kernel_source_sha():
    """Identity of the convolution kernels' source (what a committed PMC profile must have been taken with)."""
    import hashlib
    h = hashlib.sha256()
    csrc = os.path.join(ROOT, "brats21_amd", "csrc")
    for name in sorted(os.listdir(csrc)):
        if (name.startswith("conv_") and name.endswith((".hip", ".hpp"))) or name == "common.hpp":
            h.update(name.encode())
            h.update(open(os.path.join(csrc, name), "rb").read())
    return h.hexdigest()[:16]


def profiled_traffic(kernel_label):
    """HBM traffic of the dominant kernel from the committed, separately collected rocprofv3 --pmc passes
    (scripts/pmc.sh + scripts/pmc_report.py --json): used only when the record names this kernel / shape AND was
    taken with the very kernel sources that are running now -- otherwise the figure would be stale and stays null."""
    import glob
    sha = kernel_source_sha()
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "*pmc_dominant.json")), reverse=True):
        try:
            rec = json.load(open(path))
        except Exception:
            continue
        if rec.get("kernel_label") == kernel_label and rec.get("source_sha16") == sha:
            return rec, os.path.relpath(path, ROOT)
    return None, None


PMC_LABEL = "conv_igemm cin=48 cout=48 k=3 dil=1 @2x128x128x128"  # the launch `--pmc-leg` repeats (= roofline.kernel of the headline)


def pmc_leg():
    """`bench.py --pmc-leg`: nothing but the dominant kernel's launch -- the 48 -> 48 3x3x3 forward of 2 x 128^3 with tile statistics,
    as the network issues it -- 2 warm-ups + 6 launches.  Run under `rocprofv3 --pmc ... -- python3 bench.py --pmc-leg` by
    live_traffic() below (or by hand); prints one line with what it launched."""
    from brats21_amd import ops
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    x = torch.relu(torch.randn(2, 128, 128, 128, 48, device=dev)).to(torch.bfloat16)
    w = torch.randn(48, 48, 3, 3, 3, device=dev) * (2.0 / (48 * 27)) ** 0.5
    wpk = ops.pack_weights(w, torch.bfloat16, ops.PACK_FWD)
    for _ in range(8):
        ops.conv3d(x, wpk, 48, 3, 1, want_stats=True)
    torch.cuda.synchronize()
    print(json.dumps({"pmc_leg": PMC_LABEL, "launches": 8}))
    return 0


def live_traffic(kernel_label):
    """HBM traffic of the dominant kernel measured IN THIS RUN of bench.py: after the timed region, two child
    processes `rocprofv3 --kernel-trace --pmc <counter> -- python3 bench.py --pmc-leg` -- FETCH_SIZE and WRITE_SIZE in separate
    passes, never combined with a system trace (MI355X_MICROARCH.md, HBM / rocprofv3 PMC slots) -- and the per-launch mean of the
    kernel's dispatches from the counter CSV; FETCH_SIZE doubled (gfx950 tallies 128-byte requests at 64 bytes), WRITE_SIZE as
    read (16-byte-per-lane stores), both in KiB.  None when the label is not this launch, rocprofv3 is missing or a pass failed --
    the committed record (profiled_traffic) is then the labelled fallback."""
    import csv, glob, shutil, subprocess, tempfile
    if kernel_label != PMC_LABEL or shutil.which("rocprofv3") is None:
        return None
    out = {}
    tmp = tempfile.mkdtemp(prefix="brats_pmc_", dir="/tmp")
    try:
        for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
            d = os.path.join(tmp, ctr)
            cmd = ["rocprofv3", "--kernel-trace", "--pmc", ctr, "--output-format", "csv", "-d", d, "--", sys.executable,
                   os.path.abspath(__file__), "--pmc-leg"]
            p = subprocess.run(cmd, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                               text=True, timeout=240)
            vals, durs = [], []
            for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
                for r in csv.DictReader(open(f)):
                    if "conv_igemm_vs8_kernel" in r["Kernel_Name"] and r["Counter_Name"] == ctr:
                        vals.append(float(r["Counter_Value"]))
                        durs.append(float(r["End_Timestamp"]) - float(r["Start_Timestamp"]))
            if p.returncode != 0 or len(vals) < 4:
                print(f"bench.py: rocprofv3 --pmc {ctr} pass gave {len(vals)} dispatches (rc {p.returncode}): {p.stdout[-400:]}", file=sys.stderr)
                return None
            vals, durs = vals[2:], durs[2:]  # (the two warm-up launches)
            out[ctr] = (sum(vals) / len(vals), sum(durs) / len(durs), len(vals))
    except Exception as e:
        print(f"bench.py: live PMC traffic failed: {e!r}", file=sys.stderr)
        return None
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return {"fetch_MB": round(2 * out["FETCH_SIZE"][0] / 1024, 1), "write_MB": round(out["WRITE_SIZE"][0] / 1024, 1),
            "launches": out["FETCH_SIZE"][2], "dur_us_under_pmc": round(out["FETCH_SIZE"][1] / 1e3, 1)}


def inference_bench(model, dev, args):
    """BASELINE.json configs[3] and the reference-faithful variants SURVEY.md 8(d) asks for, one synthetic 4x240x240x155
    volume (padded to a multiple of 8 like learning/engine.py:217 -> 160), everything on the GPU (fused gather,
    hipGraph-replayed patch step without the deep heads, fused de-augment + sigmoid + accumulate, on-GPU mean + threshold
    + background removal + BraTS labels + crop):
      * "inference"              : 128^3 window, overlap 0.5 (18 windows), 8-flip TTA = 144 patch forwards (configs[3]);
      * "inference_ref16"        : the reference's own 16 TTA transforms (src/definer.py:647-658) x overlap 0.25 (the
                                   inferer's default, utils/inferers.py:31) = 288 patch forwards;
      * "inference_whole_volume" : the reference's published evaluation path -- no sliding window, the whole padded volume
                                   through the network, 16 TTA transforms (learning/engine.py:305-309, README.md:134-170)."""
    from brats21_amd import synth, tta
    from brats21_amd.evaluate import Evaluator
    model.eval()
    model.skip_deep_heads_in_eval = True
    amp = args.precision not in ("fp32", "x3")
    amp_dtype = torch.float16 if args.precision == "fp16" else torch.bfloat16
    vol = synth.random_image(1, 4, (240, 240, 155), seed=99, device=dev)
    vol = vol * (synth.nested_spheres(1, (240, 240, 155), device=dev)[:, 0:1] > 0)  # zero background outside the "brain"
    fwd_flop = 1995.7e9 if args.model == "equiunet" else 1689.8e9  # per 4x128^3 patch forward
    legs = {}

    def leg(name, transforms, roi, overlap, forwards, flop, what, leg_amp=None):
        transforms = list(transforms)
        ev = Evaluator(model, tta_transforms=transforms, sliding_window_size=roi, sw_batch_size=args.sw_batch, overlap=overlap,
                       k_divisible=8, amp=amp if leg_amp is None else leg_amp, use_graph=True, amp_dtype=amp_dtype)
        with torch.no_grad():
            ev(vol)  # warm-up: lazy init, allocator, graph capture of every patch / volume shape
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = ev(vol, want_labels=True)
            torch.cuda.synchronize()
            sec = time.perf_counter() - t0
        assert tuple(out["labels"].shape) == (1, 1, 240, 240, 155)
        legs[name] = {"metric": "inference volumes/sec", "value": round(1.0 / sec, 4), "unit": "volumes/s", "config": what,
                      "s_per_volume": round(sec, 3), "forwards": forwards, "ms_per_forward": round(sec / forwards * 1e3, 2),
                      "TFLOPs": round(flop / sec / 1e12, 1),
                      "foreground_fraction": round(float((out["labels"] != 0).float().mean()), 5)}
        del ev

    roi = (128, 128, 128)
    with torch.no_grad():  # first touch outside any graph (allocator, lazy init)
        Evaluator(model, tta_transforms=tta.flip8()[:1], sliding_window_size=roi, overlap=0.5, amp=amp, use_graph=False, amp_dtype=amp_dtype)(vol)
    leg("inference", tta.flip8(), roi, 0.5, 144, 144 * fwd_flop,
        f"4x240x240x155 padded to 160 (learning/engine.py:217), window 128^3, overlap 0.5, 18 windows x 8-flip TTA = 144 patch "
        f"forwards ({args.sw_batch} windows per launch), {args.precision}, hipGraph patch step, on-GPU mean + threshold + "
        "background removal + BraTS labels + crop")
    if amp and not args.fp8:
        # configs[3] in the 1e-3-logit parity mode: f32 tensors, 3x3x3 convolutions on three fp16-pair MFMA products
        old_prec, model.precision = model.precision, "x3"
        try:
            leg("inference_x3", tta.flip8(), roi, 0.5, 144, 144 * fwd_flop,
                "the same volume / windows / 8-flip TTA as `inference`, model.precision='x3' (f32 storage, split-precision "
                "convolutions: stitched logits within 1e-3 of the CPU oracle, tests/test_config3_gpu.py)", leg_amp=False)
        finally:
            model.precision = old_prec
    if not args.infer_headline_only:
        leg("inference_ref16", tta.get_tta_transforms(), roi, 0.25, 288, 288 * fwd_flop,
            "same volume, window 128^3, overlap 0.25 (18 windows), the reference's 16 TTA transforms (src/definer.py:647-658) "
            f"= 288 patch forwards, {args.precision}")
        vox = 240 * 240 * 160 / 128.0 ** 3
        leg("inference_whole_volume", tta.get_tta_transforms(), None, 0.25, 16, 16 * vox * fwd_flop,
            "same volume, NO sliding window: the whole padded 240x240x160 volume through the network, 16 TTA transforms (the "
            f"reference's published evaluation path, learning/engine.py:305-309), {args.precision}, one hipGraph per volume shape")
    model.train()
    model.skip_deep_heads_in_eval = False
    return legs


def rank_cpu_sets(n):
    """Disjoint CPU sets for the n ranks of this node: the CPUs this process may run on (sched_getaffinity), dealt out in
    n contiguous slices (contiguous ids share a core complex / NUMA node on the EPYC hosts of MI355X nodes).  A rank whose
    enqueue thread migrates between sockets, or eight ranks' OpenMP pools each spawning one thread per core, is the classic
    way a launch-bound eager step loses its scaling.  None when there are fewer CPUs than ranks."""
    cpus = sorted(os.sched_getaffinity(0))
    per = len(cpus) // n
    if per < 1:
        return None
    return [cpus[r * per:(r + 1) * per] for r in range(n)]


def _cpulist(text):
    out = []
    for part in text.strip().split(","):
        if "-" in part:
            a, b = part.split("-")
            out += list(range(int(a), int(b) + 1))
        elif part:
            out.append(int(part))
    return out


def gpu_local_cpus():
    """Per GPU of this node (KFD node order = HIP device order when no *_VISIBLE_DEVICES mask reorders it): the CPUs of the NUMA
    node its PCIe root hangs off, from /sys/bus/pci/devices/<domain:bus:dev.fn>/local_cpulist.  sysfs only, no HIP call.
    None when the topology cannot be read."""
    import glob
    out = []
    nodes = sorted(glob.glob(os.path.join(KFD_NODES, "*", "properties")), key=lambda p: int(p.split("/")[-2]))
    for p in nodes:
        try:
            props = dict(line.split()[:2] for line in open(p) if len(line.split()) >= 2)
            if int(props.get("simd_count", "0")) <= 0:
                continue
        except PermissionError:
            continue  # (another container's GPU)
        except (OSError, ValueError):
            return None
        try:
            loc, dom = int(props["location_id"]), int(props.get("domain", "0"))
            bdf = f"{dom:04x}:{(loc >> 8) & 0xff:02x}:{(loc >> 3) & 0x1f:02x}.{loc & 7:x}"
            out.append(_cpulist(open(os.path.join(PCI_DEVICES, bdf, "local_cpulist")).read()))
        except (OSError, KeyError, ValueError):
            return None
    return out or None


def pin_rank_to_cpus():
    """Called by every rank BEFORE its first GPU call: give this rank its own CPU set (process affinity + torch thread count).
    Source, in order: BRATS_RANK_CPUS from launch_ranks; else (started by somebody else's torch.distributed.run) the slice is
    computed here from LOCAL_RANK / LOCAL_WORLD_SIZE -- among the CPUs next to this rank's GPU when sysfs tells (and no device
    mask is in force), else a contiguous slice of the affinity set.  Nothing is pinned when a rank would get fewer than 4 CPUs.
    Returns {"cpus": "a-b", "n": count, "source": ...} or None."""
    local = int(os.environ.get("LOCAL_RANK", "0"))
    nloc = int(os.environ.get("LOCAL_WORLD_SIZE", os.environ.get("WORLD_SIZE", "1")))
    if os.environ.get("BRATS_NO_PIN") or nloc <= 1:
        return None
    mine, source = None, None
    spec = os.environ.get("BRATS_RANK_CPUS")
    if spec:
        sets = spec.split(";")
        if local < len(sets) and sets[local]:
            mine, source = [int(c) for c in sets[local].split(",")], "launcher (BRATS_RANK_CPUS)"
    if mine is None:
        allowed = sorted(os.sched_getaffinity(0))
        masked = any(os.environ.get(v) is not None for v in ("ROCR_VISIBLE_DEVICES", "HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"))
        near = None if masked else gpu_local_cpus()
        if near is not None and len(near) == nloc:
            # the ranks whose GPUs share a NUMA node split that node's CPUs between them, in rank order
            key = tuple(near[local])
            peers = [r for r in range(nloc) if tuple(near[r]) == key]
            pool = [c for c in near[local] if c in set(allowed)]
            per = len(pool) // len(peers)
            if per >= 4:
                i = peers.index(local)
                mine, source = pool[i * per:(i + 1) * per], "CPUs of the GPU's NUMA node (sysfs local_cpulist), split between its ranks"
        if mine is None:
            sets = rank_cpu_sets(nloc)
            if sets is not None:
                mine, source = sets[local], "contiguous slice of the affinity set"
    if not mine or len(mine) < 4:  # (an enqueue thread + the runtime's and RCCL's helper threads on fewer CPUs: worse than no pin)
        return None
    try:
        os.sched_setaffinity(0, set(mine))
    except OSError:
        return None
    torch.set_num_threads(max(1, min(8, len(mine))))
    return {"cpus": f"{min(mine)}-{max(mine)}" if mine == list(range(min(mine), max(mine) + 1)) else ",".join(map(str, mine)),
            "n": len(mine), "source": source}


_RANK_ENV = ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "GROUP_RANK", "GROUP_WORLD_SIZE", "ROLE_RANK", "ROLE_NAME",
             "ROLE_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "TORCHELASTIC_RESTART_COUNT", "TORCHELASTIC_MAX_RESTARTS",
             "TORCHELASTIC_RUN_ID", "TORCHELASTIC_USE_AGENT_STORE", "TORCHELASTIC_ERROR_FILE", "TORCH_NCCL_ASYNC_ERROR_HANDLING",
             "BRATS_RANK_CPUS")


def run_ranks(n, argv, env, timeout_s):
    """One `python -m torch.distributed.run` child over n ranks, in its own process group (on a timeout exactly that group is
    killed -- the agent AND its rank processes); returns (rc, [JSON lines of rank 0], other stdout lines).  rc 124 = timed out."""
    import signal
    import socket
    import subprocess
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
    proc = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, text=True, start_new_session=True)
    try:
        out, _ = proc.communicate(timeout=timeout_s)
        rc = proc.returncode
    except subprocess.TimeoutExpired:
        try:
            os.killpg(proc.pid, signal.SIGKILL)  # (start_new_session: the child's pid is its process-group id)
        except ProcessLookupError:
            pass
        out, _ = proc.communicate()
        rc = 124
    out = out or ""
    js = [l for l in out.splitlines() if l.lstrip().startswith("{")]
    other = [l for l in out.splitlines() if not l.lstrip().startswith("{")]
    return rc, js, other


def graph_ddp_leg(n, argv, base_env):
    """The second leg of an N > 1 run, in FRESH rank processes (a child torch.distributed.run of the caller): the same workload
    with the whole step -- forward, fused Dice, the backward program pushing into the gradient buckets, the buckets' RCCL
    all-reduces, Ranger2020 -- captured once and replayed as ONE hipGraph per rank (--graph, BRATS_GRAPH_DDP=1).  One launch per
    step takes the ~400 kernel enqueues per step off every rank's host thread, which is what decides the scaling when the
    eager step is enqueue-bound (compare host_enqueue_ms with ms_per_step).  This path has never run on more than one GPU (this
    pool has 1-GPU boxes): it can only ADD information.  Returns the "graph_ddp" record: rc 0 + its numbers, or the exit code
    (124 = timed out and killed) + the tail of what it said; it is never retried and cannot change the eager headline."""
    env = {k: v for k, v in base_env.items() if k not in _RANK_ENV}
    env["BRATS_GRAPH_DDP"] = "1"
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    drop = {"--graph", "--no-graph-leg", "--kernel-table"}
    leg_argv = [a for a in argv if a not in drop] + ["--graph", "--no-graph-leg", "--no-cpu-baseline"]
    t0 = time.perf_counter()
    try:
        rc, js, other = run_ranks(n, leg_argv, env, float(base_env.get("BRATS_GRAPH_LEG_TIMEOUT", "300")))
    except Exception as e:
        return {"rc": -1, "error": repr(e)[:300]}
    leg = {"rc": rc, "wall_s": round(time.perf_counter() - t0, 1),
           "what": "same workload, whole step incl. the bucketed RCCL all-reduces replayed as ONE hipGraph per rank (--graph, "
                   "BRATS_GRAPH_DDP=1) in fresh rank processes after the eager headline; rc != 0: the capture / replay failed "
                   "(124: hung, killed) and was not retried"}
    if rc == 0 and js:
        g = json.loads(js[-1])
        leg.update({"ms_per_step": g.get("ms_per_step"), "value": g.get("value"), "unit": g.get("unit"), "n_gpus": g.get("n_gpus"),
                    "host_enqueue_ms": g.get("host_enqueue_ms"), "loss": g.get("config", {}).get("loss"), "ddp": g.get("ddp")})
    else:
        leg["stdout_tail"] = " | ".join(other[-6:])[-800:]
    return leg


def launch_ranks(n, argv, dry_run=False):
    """Started bare with --gpus N: run the N ranks as CHILD processes of this one, which never touches the GPU.
    Leg 1 (the headline) is the eager data-parallel step; its JSON line is the line of this run.  Leg 2 (graph_ddp_leg) runs only
    under --full, after leg 1 succeeded and only for the default eager headline, and lands on the line as "graph_ddp"."""
    if not dry_run and os.environ.get("BRATS_DIST_BACKEND") != "gloo":  # (gloo: the debugging set-up with ranks sharing a GPU)
        have = gpu_count_without_hip()  # (sysfs; unknown -> the ranks' own device / WORLD_SIZE checks fail loudly instead)
        if have is not None and have < n:
            print(f"bench.py: --gpus {n} but this node has {have} GPU(s)", file=sys.stderr)
            return 2
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "8")  # (each rank narrows its own torch pool to its CPU slice: pin_rank_to_cpus)
    want_graph_leg = not dry_run and "--full" in argv and "--graph" not in argv and "--no-graph-leg" not in argv \
        and env.get("BRATS_DIST_BACKEND") != "gloo"
    rc, js, other = run_ranks(n, list(argv) + (["--no-graph-leg"] if want_graph_leg else []), env,
                              float(env.get("BRATS_LEG_TIMEOUT", "1800")))
    for line in other:
        print(line, file=sys.stderr)
    line = js[-1] if js else None
    if rc == 0 and line is not None and want_graph_leg:
        try:
            rec = json.loads(line)
            rec["graph_ddp"] = graph_ddp_leg(n, argv, env)
            line = json.dumps(rec)
        except Exception as e:  # the headline line must get out whatever the extra leg did
            print(f"bench.py: graph leg bookkeeping failed: {e!r}", file=sys.stderr)
    if line is not None:
        print(line)
    sys.stdout.flush()
    return rc


def dry_run(args):
    """--dry-run: rendezvous + one CPU all-reduce over gloo, no GPU."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the process group has WORLD_SIZE={world}")
    total = 1.0
    if world > 1:
        dist.init_process_group(backend="gloo", rank=rank, world_size=world)
        v = torch.ones(1)
        dist.all_reduce(v)
        total = float(v.item())
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        print(json.dumps({"metric": "dry run", "n_gpus": world, "dry_run": True, "ranks_seen": int(total)}))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # defaults: 20 + 50 steps = 1.1 s of training; the first ~20 steps after start-up run 1-2 % slower than the steady state
    # (clock / power management settling: 16.0 -> 15.8 ms measured step by step), so a 3 + 10 run reads ~0.2 ms high
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--width", type=int, default=48)
    ap.add_argument("--batch", type=int, default=2, help="patches per GPU")
    ap.add_argument("--patch", type=int, default=128)
    ap.add_argument("--model", default="equiunet")
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp16", "fp32", "x3"],
                    help="fp16 = the reference's own autocast dtype (IEEE half storage) under its GradScaler loop; bf16 is the headline; "
                         "fp32 = exact-f32 MFMA kernels; x3 = f32 storage with split-precision (3 x fp16-pair MFMA) convolutions")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-parity-leg", action="store_true", help="skip the fp32 (1e-3 logit parity) timing leg")
    ap.add_argument("--no-infer", action="store_true", help="skip the sliding-window + TTA inference measurement")
    ap.add_argument("--other-configs-patch", type=int, default=0, help="(tests) run the other-configuration legs at this patch size")
    ap.add_argument("--no-other-configs", action="store_true",
                    help="skip the short legs of the other stated configurations (configs2_per_gpu, fp16_mode, configs4_per_gpu)")
    ap.add_argument("--infer-headline-only", action="store_true", help="only the configs[3] inference leg (8-flip, overlap 0.5)")
    ap.add_argument("--torch-dice", dest="fused_dice", action="store_false",
                    help="use the PyTorch Dice loss (reference path) instead of the fused HIP Dice passes")
    ap.add_argument("--optimizer", default="ranger", choices=["ranger", "adam"],
                    help="ranger = the reference's default (--optimizer ranger, src/arguments_train.py:120), fused HIP step")
    ap.add_argument("--use-gc", action="store_true", help="Ranger gradient centralisation (reference default: off)")
    ap.add_argument("--sw-batch", type=int, default=4, help="sliding-window windows per forward in the inference leg")
    ap.add_argument("--graph", action="store_true",
                    help="replay the whole step as one hipGraph (single GPU; no per-kernel timers, so roofline is null)")
    ap.add_argument("--fp8", default=None, choices=["fwd", "all"],
                    help="NOT the headline configuration: run the 3x3x3 convolutions forward (fwd) or forward + input "
                         "gradients (all) on the e4m3 MFMA kernel (BASELINE.json configs[4]); weight gradients stay bf16")
    ap.add_argument("--dropout", type=float, default=0.0, help="NOT the headline configuration: --dropout p of the reference's CLI")
    ap.add_argument("--kernel-table", action="store_true", help="print the per-kernel time table (rank 0; needs --full)")
    ap.add_argument("--no-pmc-traffic", action="store_true",
                    help="do not measure roofline.traffic in this run (two rocprofv3 --pmc child processes after the timed region)")
    ap.add_argument("--pmc-leg", action="store_true", help="(internal) only the dominant kernel's launch, for a rocprofv3 --pmc pass")
    ap.add_argument("--no-graph-leg", action="store_true",
                    help="bare --gpus N > 1: do not run the second leg (the step incl. its RCCL all-reduces as one hipGraph, fresh ranks)")
    ap.add_argument("--full", action="store_true",
                    help="measure everything besides the headline (box probe, roofline + live PMC traffic, host-enqueue / ddp "
                         "accounting, inference, parity mode, other configurations, CPU baseline, the N > 1 graph leg); the "
                         "--no-* switches above narrow it")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's loss and the updated parameters / gradients (fixed sample of the large "
                         "ones) as float32 .npy files under DIR (rank 0)")
    ap.add_argument("--dry-run", action="store_true",
                    help="launcher / rendezvous check only: every rank joins the process group (gloo on CPU), one all-reduce, rank 0 "
                         "prints {n_gpus, dry_run}; no GPU is touched (tests/test_bench_launch_cpu.py)")
    args = ap.parse_args()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # started bare with --gpus N: start the N ranks ourselves, as a CHILD process, before anything touches the GPU (a
        # process that has initialised the GPU must never exec another program on this pool), and relay rank 0's JSON line
        sys.exit(launch_ranks(args.gpus, sys.argv[1:], dry_run=args.dry_run))
    if args.dry_run:
        return dry_run(args)
    if args.pmc_leg:
        return pmc_leg()
    # stdout carries ONE JSON line: everything else this process and its libraries print from here on (RCCL's version banner goes
    # to fd 1 at communicator creation) is sent to stderr; emit() below writes the line to the real stdout
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)

    def emit(obj):
        os.write(real_stdout, (json.dumps(obj) + "\n").encode())

    from brats21_amd import get_model, ops, LIB_PATH
    from brats21_amd import synth
    from brats21_amd.ddp import GradientBuckets, init_process_group_from_env
    from brats21_amd.engine import TrainStep
    from brats21_amd.losses import DiceLoss
    from brats21_amd.optim import Ranger2020

    assert os.path.exists(LIB_PATH), "HIP extension missing"
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # (dmabuf IPC: RCCL's peer buffers need it on these hosts)
    try:
        pin = pin_rank_to_cpus()  # before the first GPU call of this rank
    except Exception as e:  # (a topology this code has not seen must never cost the run)
        print(f"bench.py: CPU pinning skipped: {e!r}", file=sys.stderr)
        pin = None
    rank, world, local = init_process_group_from_env()
    if world != args.gpus:  # never measure world 1 under an n_gpus = N label
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the process group has WORLD_SIZE={world}")
    local = local % max(torch.cuda.device_count(), 1)  # (two ranks may share one GPU under BRATS_DIST_BACKEND=gloo)
    torch.cuda.set_device(local)
    # BRATS_FORCE_DDP=rccl at world 1: the REHEARSAL of an N > 1 run on a 1-GPU box -- a real RCCL communicator over one rank,
    # every bucket's all-reduce a real asynchronous RCCL launch, the whole `ddp` block and the graph leg of the line exercised
    rehearsal = world == 1 and os.environ.get("BRATS_FORCE_DDP") == "rccl"
    if rehearsal and not dist.is_initialized():
        import socket
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if "MASTER_PORT" not in os.environ:
            with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
                sk.bind(("127.0.0.1", 0))
                os.environ["MASTER_PORT"] = str(sk.getsockname()[1])
        dist.init_process_group("nccl", rank=0, world_size=1)
    live = dist.is_initialized()  # collectives of the accounting below run whenever there is a process group
    dev = torch.device("cuda", local)
    torch.manual_seed(0)  # identical random-init weights on every rank
    ns = argparse.Namespace(model=args.model, width=args.width, norm="group", act="relu", num_classes=3, dropout=args.dropout)
    import contextlib, io
    with contextlib.redirect_stdout(io.StringIO()):
        model = get_model(ns).to(dev).train()
    if args.fp8:
        assert args.precision in ("bf16", "fp16"), "--fp8 needs 16-bit activations"
        model.conv_fp8 = args.fp8
    crit = DiceLoss().to(dev)
    if args.optimizer == "ranger":  # src/definer.py:316-331 + the CLI defaults lr 1e-4, weight_decay 1e-5
        with contextlib.redirect_stdout(io.StringIO()):
            opt = Ranger2020(model.parameters(), lr=1e-4, alpha=0.5, k=6, N_sma_threshhold=5, betas=(.95, 0.999), eps=1e-5,
                             weight_decay=1e-5, use_gc=args.use_gc, capturable=args.graph or args.precision == "fp16")
    else:
        opt = torch.optim.Adam(model.parameters(), lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-5, foreach=True)
    buckets = GradientBuckets(model) if (world > 1 or os.environ.get("BRATS_FORCE_DDP")) else None  # BRATS_DDP_BF16=1: bf16 transport
    if rehearsal:
        buckets.force_collectives = True
    size = (args.patch,) * 3
    x = synth.random_image(args.batch, 4, size, seed=1234 + rank, device=dev)
    t = synth.nested_spheres(args.batch, size, device=dev)
    use_amp = args.precision not in ("fp32", "x3")
    if args.precision == "x3":
        model.precision = "x3"
    amp_dtype = torch.float16 if args.precision == "fp16" else torch.bfloat16
    train_step = TrainStep(model, opt, criterion=None if args.fused_dice else crit, amp=use_amp, buckets=buckets, amp_dtype=amp_dtype)

    if args.graph:  # (with N > 1 the bucketed RCCL all-reduces are captured into the graph too)
        assert args.optimizer == "ranger", "--graph: ranger optimizer (capturable)"
        from brats21_amd.engine import GraphedTrainStep
        # world > 1: RCCL inside the capture is unverified on multi-GPU hardware -> explicit opt-in (BRATS_GRAPH_DDP=1)
        train_step = GraphedTrainStep(train_step, warmup=2)

    def step():
        return train_step(x, t)

    for _ in range(args.warmup):
        step()
    # what THIS box delivers right now (dense bf16 MFMA rate with every SIMD issuing, bf16 read + write stream): ~50 ms of
    # probes right before the timed region, so that a reader can tell a slower box from slower code (roofline.frac_of_box)
    box = ops.probe_box(dev) if args.full and rank == 0 else None
    timer = ops.KernelTimer() if args.full and rank == 0 and not args.graph and not os.environ.get("BRATS_BENCH_NO_TIMER") else None
    # per-kernel HIP events cost GPU time themselves (0.28 ms per step when every conv launch of every step is bracketed):
    # they are recorded in two of the timed steps only (at 1/3 and 2/3 of the run), inside the timed region, and only under --full
    sample_at = sorted({args.steps // 3, (2 * args.steps) // 3}) if args.full else []
    sampled = len(sample_at)
    def barrier():  # (RCCL: name the device, or ProcessGroupNCCL guesses it from the rank and warns)
        if dist.get_backend() == "nccl":
            dist.barrier(device_ids=[local])
        else:
            dist.barrier()

    if live:
        barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        ops.TIMER = timer if (timer is not None and i in sample_at) else None
        if buckets is not None and not args.graph:
            buckets.measure = i in sample_at  # two HIP events around the collective waits of the sampled steps
        loss = step()
    torch.cuda.synchronize()
    if live:
        barrier()
    elapsed = time.perf_counter() - t0
    ops.TIMER = None
    mine_elapsed = elapsed
    if live:  # the headline quantity first: MAX over ranks of the timed region (everything below is accounting around it)
        el = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(el, op=dist.ReduceOp.MAX)
        elapsed = float(el.item())
    if args.dump_outputs and rank == 0:  # (before anything below runs another step)
        dump_outputs(args.dump_outputs, loss, model)
    # host side of a step, measured AFTER the timed region on an empty queue: how long this rank's Python / launch path needs to
    # enqueue three steps while the GPU is still busy with the first (inside the 50-step region the enqueue thread runs into the
    # full HIP queue and its time converges to the GPU's).  host_enqueue_ms close to ms_per_step = the eager step is bound by the
    # host, and eight ranks on one host scale by their CPUs, not by their GPUs -- the case the graph leg (one launch per step) is for
    if buckets is not None:
        buckets.measure = False
    host_enqueue_ms = None
    if args.full:
        th = time.perf_counter()
        for _ in range(3):
            step()
        host_enqueue_ms = (time.perf_counter() - th) / 3 * 1e3
        torch.cuda.synchronize()
    ddp_info = None
    if buckets is not None and args.full:
      try:  # (accounting only: whatever goes wrong here must not cost the line its headline)
          # data-parallel accounting: per-rank step time, the collectives' stand-alone cost, and how much of it the overlap
          # with the backward kernels hid (exposed = GPU time finish() waited for them in the sampled steps)
          # (nothing is sampled under --graph: timing events cannot be recorded into a replayed graph -> exposed / overlap
          #  are reported as null, never as a made-up 0.0 / 1.0)
          exp_mine = buckets.exposed_ms()
          mine = torch.tensor([mine_elapsed / args.steps * 1e3, float("nan") if exp_mine is None else exp_mine, host_enqueue_ms,
                               float(pin["n"]) if pin else 0.0], device=dev, dtype=torch.float64)
          # ranks_seen: a 1 from every rank summed by the collective library itself (what the job's RCCL communicator spans)
          ones = torch.ones(1, device=dev, dtype=torch.float32)
          if live:
              dist.all_reduce(ones)
              both = [torch.empty_like(mine) for _ in range(world)]
              dist.all_gather(both, mine)
          else:
              both = [mine]
          ar = buckets.allreduce_ms()
          exps = [float(b[1]) for b in both]
          exposed = None if any(e != e for e in exps) else max(exps)  # NaN = not measured on that rank
          ddp_info = {"world_size": dist.get_world_size() if dist.is_initialized() else 1, "ranks_seen": int(round(float(ones.item()))),
                      "backend": dist.get_backend() if dist.is_initialized() else None,
                      "rccl_version": ".".join(str(v) for v in torch.cuda.nccl.version()) if hasattr(torch.cuda, "nccl") else None,
                      "ms_per_step_by_rank": [round(float(b[0]), 3) for b in both],
                      "host_enqueue_ms_by_rank": [round(float(b[2]), 3) for b in both],
                      "host_enqueue_ms": round(max(float(b[2]) for b in both), 3),
                      "cpus_per_rank": [int(b[3]) for b in both], "cpu_pinning_rank0": pin,
                      "buckets": len(buckets._plan),
                      "payload_MB": round(buckets.payload_bytes() / 1e6, 1), "comm_dtype": str(buckets.comm_dtype).replace("torch.", ""),
                      "allreduce_ms": round(ar, 3), "exposed_ms": None if exposed is None else round(exposed, 3),
                      "overlap_frac": round(max(0.0, 1.0 - exposed / ar), 3) if (ar > 0 and exposed is not None) else None,
                      "graph_captured_collectives": bool(args.graph)}
      except Exception as e:
        ddp_info = {"error": repr(e)[:300]}
    if rank != 0:
        if live:
            dist.destroy_process_group()
        return

    # ---- roofline of the dominant kernel, from HIP events recorded inside the timed steps ----
    if timer is None:  # --graph: one graph launch per step, no per-kernel HIP events
        roofline = None
        table = {}
    else:
        table = timer.summary()
    fam = {}
    for key, (cnt, avg, tot) in table.items():
        fam.setdefault(key[0], [0.0, 0.0])
        kind, cin, cout, k, dil, n, d, h, w, dt = key
        fam[kind][0] += tot
        fam[kind][1] += conv_flops(cin, cout, k, n, d, h, w) * cnt
    if table:
      # The roofline line is about a launch whose WHOLE work is the algorithmic FLOPs in its numerator.  Launches of the
      # "backward statistics" form (family conv_igemm_bst: the same implicit GEMM whose epilogue also does the first pass of a
      # GroupNorm backward, replacing a separate HBM-bound kernel) are listed beside it (`fused_epilogue_form`), not as it.
      plain = [k for k in table if not k[0].endswith("_bst")]
      dom_key = max(plain or list(table), key=lambda k: table[k][2])
      cnt, avg_ms, tot_ms = table[dom_key]
      kind, cin, cout, k, dil, n, d, h, w, dt = dom_key
      fl = conv_flops(cin, cout, k, n, d, h, w)
      # (x3: three 16-bit MFMAs per algorithmic product -- the kernel's ceiling is a third of the 16-bit peak)
      x3 = dt.startswith("x3")
      peak = PEAK_FP8_TFLOPS if dt == "e4m3" else (PEAK_BF16_TFLOPS / 3 if x3 else (PEAK_BF16_TFLOPS if use_amp else PEAK_F32_TFLOPS))
      achieved = fl / (avg_ms * 1e-3) / 1e12
      # frac_of_box: against the matrix rate this chip SUSTAINED in the probe right before the timed region (dense operands, every
      # SIMD issuing; e4m3 runs at twice, exact f32 at 1/16 of the 16-bit pipe rate) -- comparable across the boxes of a pool,
      # which frac (against the nominal peak at 2.4 GHz) is not
      box_peak = box["mfma_TFLOPs"] * (2.0 if dt == "e4m3" else (1.0 / 3 if x3 else (1.0 if use_amp else PEAK_F32_TFLOPS / PEAK_BF16_TFLOPS)))
      roofline = {"bound": "mfma", "kernel": f"{kind} cin={cin} cout={cout} k={k} dil={dil} @{n}x{d}x{h}x{w}",
                  "achieved": round(achieved, 2), "peak": peak, "unit": "TFLOP/s", "frac": round(achieved / peak, 4),
                  "frac_of_box": round(achieved / box_peak, 4),
                  "traffic": None, "launches": cnt, "avg_ms": round(avg_ms, 4),
                  "sampled_steps": sampled,
                  "families": {f: {"ms_per_step": round(v[0] / sampled, 3), "TFLOPs": round(v[1] / (v[0] * 1e-3) / 1e12, 1)}
                               for f, v in fam.items()}}
      fused = [k for k in table if k[0].endswith("_bst")]
      if fused:
          fk = max(fused, key=lambda k: table[k][2])
          fcnt, favg, _ = table[fk]
          ffl = conv_flops(fk[1], fk[2], fk[3], fk[5], fk[6], fk[7], fk[8])
          roofline["fused_epilogue_form"] = {
              "kernel": f"{fk[0]} cin={fk[1]} cout={fk[2]} k={fk[3]} dil={fk[4]} @{fk[5]}x{fk[6]}x{fk[7]}x{fk[8]}", "launches": fcnt,
              "avg_ms": round(favg, 4), "achieved": round(ffl / (favg * 1e-3) / 1e12, 2), "frac": round(ffl / (favg * 1e-3) / 1e12 / peak, 4),
              "note": "the same implicit GEMM with GroupNorm backward's first pass (sum u, sum u*y per tile and channel) in its epilogue "
                      "(brats_conv3d_fwd_bstats): the separate pass it replaces cost 0.15 ms at this shape; model.fold_bwd_stats"}
    # HBM traffic of the dominant kernel comes from separate --pmc passes (never collected inside this timed run):
    # `traffic` is the committed per-launch figure of those passes, null unless it was taken on this kernel, this shape
    # and these kernel sources (profiled_traffic)
    pmc_now = None
    if roofline is not None and world == 1 and not args.no_pmc_traffic and not args.graph:
        pmc_now = live_traffic(roofline["kernel"])
    if pmc_now is not None:
        n_, d_, h_, w_ = 2, 128, 128, 128
        roofline["traffic"] = int((pmc_now["fetch_MB"] + pmc_now["write_MB"]) * 1024 * 1024)  # bytes per launch
        roofline["traffic_profiled"] = dict(pmc_now, algorithmic_MB=round(2 * (n_ * d_ * h_ * w_ * 48 * 2) / 1e6, 1),
                                            source="live: rocprofv3 --kernel-trace --pmc FETCH_SIZE / WRITE_SIZE in two child processes "
                                                   "of THIS run (bench.py --pmc-leg: the same launch, 6 dispatches averaged), MiB per "
                                                   "launch, FETCH_SIZE doubled per MI355X_MICROARCH.md")
    elif roofline is not None:
        rec, src = profiled_traffic(roofline["kernel"])
        if rec is not None:
            roofline["traffic"] = int((rec["fetch_MB"] + rec["write_MB"]) * 1024 * 1024)  # bytes per launch (the report prints MiB)
            roofline["traffic_profiled"] = {"fetch_MB": rec["fetch_MB"], "write_MB": rec["write_MB"],
                                            "algorithmic_MB": round(2 * (n * d * h * w * cout * 2) / 1e6, 1),
                                            "source": "committed record (no live measurement in this run): " + src + " (rocprofv3 --pmc, separate passes over this kernel and shape, per launch; "
                                                            "FETCH_SIZE doubled per MI355X_MICROARCH.md)"}
    if args.kernel_table:
        for key in sorted(table, key=lambda k: -table[k][2]):
            c, a, tt = table[key]
            kk, ci, co, ks, dl, nn, dd, hh, ww, dt = key
            tf = conv_flops(ci, co, ks, nn, dd, hh, ww) / (a * 1e-3) / 1e12
            print(f"# {kk:11s} cin={ci:4d} cout={co:4d} d={dl} @{dd:3d}^3  n={c:3d} avg {a:8.3f} ms  {tf:7.1f} TF/s  total {tt:8.2f} ms",
                  file=sys.stderr)
    patches = world * args.batch * args.steps
    res = {
        "metric": f"train patches/sec (4x{args.patch}^3, width-{args.width})", "value": round(patches / elapsed, 4), "unit": "patches/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 2),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": args.precision + (f"+e4m3 conv ({args.fp8})" if args.fp8 else ""), "data": "synthetic",
        "config": {"workload": f"{args.model} width={args.width}, batch={args.batch}/GPU of 4x{args.patch}^3 synthetic patches, "
                               f"fwd + deep-supervision Dice + bwd + {args.optimizer}" + (" as one hipGraph" if args.graph else "") +
                               (f", dropout {args.dropout}" if args.dropout else "") +
                               (" (BASELINE.json configs[1])" if (args.model, args.width, args.fp8, args.dropout) == ("equiunet", 48, None, 0.0) else
                                " (BASELINE.json configs[2], per-GPU share)" if (args.model, args.width, args.fp8) == ("equiunet_assp_evo", 48, None) else
                                f" (BASELINE.json configs[4], per-GPU share at {args.batch} patches, {args.precision} storage)" if (args.model, args.width) == ("equiunet_assp_evo", 64) and args.fp8 else ""),
                   "global_batch": world * args.batch, "parallelism": f"dp{world}", "loss": round(float(loss.item()), 5)},
    }
    if args.full:
        res.update({"host_enqueue_ms": round(host_enqueue_ms, 2), "roofline": roofline, "box": box})
    if ddp_info is not None:
        res["ddp"] = ddp_info
    legs = args.full and world == 1  # (the legs below run after the headline, on this process's GPU)
    if legs and not args.no_infer:
        res.update(inference_bench(model, dev, args))
    if legs and not args.no_parity_leg and args.precision == "bf16" and not args.fp8:
        res["parity_mode"] = parity_mode_leg(args, dev, x, t)
        res["dtype_note"] = ("value is measured in bf16 storage / f32 accumulate: logits NOT within 1e-3 (max ~0.3 on |logits| <= 28; the 1e-3-logit "
                             "configuration is parity_mode).  Hard Dice against the CPU oracle on TRAINED weights (tests/test_trained_gpu.py, six weight sets "
                             "per network, profiles/r06_final_trained_weights_parity.txt; bar 1e-3): on training-like 128^3 volumes bf16 <= 4.6e-4, fp16 <= "
                             "1.3e-4, < 5e-5 stitched over a configs[3] volume -- asserted for every weight set; on stress volumes (half / a third of the "
                             "training contrast, where the network itself is unsure) fp16 stays <= 6.1e-4 on all 20, bf16 exceeds 1e-3 on 6 of 20 (max "
                             "4.3e-3): fp16_mode, the reference's own autocast dtype, is the configuration that holds the bar there")
    if legs and not args.no_other_configs and (args.model, args.width, args.precision, args.fp8, args.batch, args.dropout) == ("equiunet", 48, "bf16", None, 2, 0.0) \
            and (args.patch == 128 or args.other_configs_patch):
        del train_step, opt
        model.zero_grad(set_to_none=True)
        torch.cuda.empty_cache()
        res.update(other_configs_legs(dev, rank, args.other_configs_patch or 128))
    if legs and not args.no_cpu_baseline:
        res["cpu_baseline"] = cpu_baseline(args.width, os.cpu_count() or 1)
    if live:
        backend = dist.get_backend()
        dist.destroy_process_group()  # (the other ranks have returned already; nothing below is collective)
        if args.full and backend == "nccl" and not args.graph and not args.no_graph_leg and not os.environ.get("BRATS_NO_GRAPH_LEG"):
            # started as a rank of somebody else's torch.distributed.run (the driver's launch form): the graph + RCCL leg runs as a
            # CHILD torch.distributed.run of rank 0 -- fresh rank processes -- after this rank gave its memory back
            train_step = opt = model = buckets = x = t = loss = crit = None  # noqa: F841 (drop every reference to device memory)
            torch.cuda.empty_cache()
            try:
                res["graph_ddp"] = graph_ddp_leg(world, sys.argv[1:], dict(os.environ))
            except Exception as e:
                res["graph_ddp"] = {"rc": -1, "error": repr(e)[:300]}
    emit(res)


if __name__ == "__main__":
    main()
