#!/usr/bin/env python3
"""Training the R3D-50 trunk (32 x 112 x 112 clips, seeded weights), events per measurement, median of --reps:

  * the trunk forward as tools/bench_r3d.py times it (frozen trunk, cached packed weights: stlt_r3d_forward), the batched weight
    repack alone (stlt_r3d_repack_all: 53 forward + 52 dgrad copies), and one trunk train step (forward with tape + backward into
    the 53 weight gradients, weights unchanged so no repack), at --batches;
  * Trainer.step clips/s for Resnet3D at 16 and 64 clips and for CACNF with the trunk at 16 (each step re-makes the copies once,
    after the optimiser moved the weights);
  * at --table-batch (16), every conv's data gradient (52: stlt_conv3d_bwd_data, the trunk's split plan) and weight gradient (53:
    stlt_conv3d_bwd_weight) launched alone, summed per class as TFLOP/s and the fraction of the 157.3 TF f32-MFMA peak, beside
    torch's MIOpen backward (aten.convolution_backward, fp32 NCDHW, input and weight gradient timed separately) on the same layers."""
import argparse, ctypes, importlib, os, sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import bench_r3d as BR  # noqa: E402  (layer table, FLOP count, event timer)

pkg = importlib.import_module("revisiting-spatial-temporal-layouts_amd")
R3D = importlib.import_module("revisiting-spatial-temporal-layouts_amd.modelling.resnet3d")
DEV = "cuda:0"
PEAK_TF = BR.PEAK_TF


def app_cfg(**kw):
    k = pkg.synth.model_kwargs("cfg1")
    return pkg.AppearanceModelConfig(num_classes=k["num_classes"], hidden_size=k["hidden_size"], num_attention_heads=k["num_attention_heads"],
                                     hidden_dropout_prob=0.0, appearance_num_frames=32, **kw)


def loaded(m):
    sd = pkg.synth.make_r3d_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=4242)
    m.load_state_dict(sd, strict=True)
    return m.to(DEV)


def trunk_table(a, lines):
    lib = pkg._lib.load()
    B = a.table_batch
    g = torch.Generator(device=DEV).manual_seed(0)
    st = torch.cuda.current_stream().cuda_stream
    per = {c: dict(n_d=0, n_w=0, gf_d=0.0, gf_w=0.0, ms_d=0.0, ms_w=0.0, mi_d=0.0, mi_w=0.0) for c in BR.CLASSES}
    rows = []
    for i, l in enumerate(BR.trunk_layers(B)):
        T, H, W = l["shape"]
        To, Ho, Wo = BR.out_shape(l)
        stem = l["cls"].startswith("stem")
        cin = 3 if stem else l["cin"]
        d = pkg._lib.Conv3dDesc(B, T, H, W, l["cin"], l["cout"], l["k"], l["k"], l["k"], *l["s"], l["p"], l["p"], l["p"])
        x = torch.rand(B, T, H, W, l["cin"], device=DEV, generator=g)
        dy = torch.randn(B, To, Ho, Wo, l["cout"], device=DEV, generator=g)
        w = torch.randn(l["cout"], cin, l["k"], l["k"], l["k"], device=DEV, generator=g) * 0.05
        dw = torch.empty_like(w)
        gf = BR.flops(B, l, 3 if stem else None) / 1e9
        wsw = torch.empty(int(lib.stlt_conv3d_bwd_weight_workspace_bytes(ctypes.byref(d), 0)), dtype=torch.uint8, device=DEV)
        ms_w = BR.time_events(lambda: pkg._lib.check(lib.stlt_conv3d_bwd_weight(ctypes.byref(d), x.data_ptr(), dy.data_ptr(), None, cin, 1, 0, wsw.data_ptr(),
                                                                                wsw.numel(), dw.data_ptr(), st), "wgrad"), a.warmup, a.reps)
        ms_d = float("nan")
        if not stem:
            wd = torch.empty(w.numel(), device=DEV)
            pkg._lib.check(lib.stlt_conv3d_repack_dgrad(w.data_ptr(), ctypes.byref(d), None, wd.data_ptr(), st), "repack_dgrad")
            nb = int(lib.stlt_conv3d_bwd_data_workspace_bytes(ctypes.byref(d), 0))
            wsd = torch.empty(max(nb, 256), dtype=torch.uint8, device=DEV)
            dx = torch.empty_like(x)
            ms_d = BR.time_events(lambda: pkg._lib.check(lib.stlt_conv3d_bwd_data(ctypes.byref(d), dy.data_ptr(), wd.data_ptr(), None, x.data_ptr(), None, 0,
                                                                                  wsd.data_ptr(), nb, dx.data_ptr(), st), "dgrad"), a.warmup, a.reps)
            del wd, wsd, dx
        mi_d = mi_w = float("nan")
        if not a.no_miopen:
            xc = x[..., :cin].permute(0, 4, 1, 2, 3).contiguous()
            dyc = dy.permute(0, 4, 1, 2, 3).contiguous()
            conv_bwd = torch.ops.aten.convolution_backward

            def mi(mask):
                return lambda: conv_bwd(dyc, xc, w, None, l["s"], [l["p"]] * 3, [1, 1, 1], False, [0, 0, 0], 1, mask)
            mi_w = BR.time_events(mi([False, True, False]), a.warmup, a.reps)
            if not stem:
                mi_d = BR.time_events(mi([True, False, False]), a.warmup, a.reps)
            del xc, dyc
        c = per[l["cls"]]
        c["n_w"] += 1; c["gf_w"] += gf; c["ms_w"] += ms_w; c["mi_w"] += mi_w
        if not stem:
            c["n_d"] += 1; c["gf_d"] += gf; c["ms_d"] += ms_d; c["mi_d"] += mi_d
        rows.append((i, l["cls"], cin, l["cout"], f"{To}x{Ho}x{Wo}", ms_d, gf / ms_d if not stem else float("nan"), ms_w, gf / ms_w, mi_d, mi_w))
        del x, dy, w, dw, wsw
    torch.cuda.empty_cache()
    lines += ["", f"Per class at B = {B} (each conv launched alone, events per launch; MIOpen = aten.convolution_backward fp32 NCDHW)", "",
              "| class | dgrad convs | dgrad ms | dgrad TFLOP/s | of peak | MIOpen dgrad ms | wgrad convs | wgrad ms | wgrad TFLOP/s | of peak | "
              "MIOpen wgrad ms |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    tot = dict(gf_d=0.0, ms_d=0.0, gf_w=0.0, ms_w=0.0, mi_d=0.0, mi_w=0.0)
    for cname in BR.CLASSES:
        c = per[cname]
        if c["n_d"]:
            dpart = f"{c['n_d']} | {c['ms_d']:.2f} | {c['gf_d'] / c['ms_d']:.1f} | {c['gf_d'] / c['ms_d'] / PEAK_TF:.3f} | {c['mi_d']:.2f}"
        else:
            dpart = "0 | – | – | – | –"
        lines.append(f"| {cname} | {dpart} | {c['n_w']} | {c['ms_w']:.2f} | {c['gf_w'] / c['ms_w']:.1f} | {c['gf_w'] / c['ms_w'] / PEAK_TF:.3f} | "
                     f"{c['mi_w']:.2f} |")
        for k in tot:
            tot[k] += c[k]
    lines.append(f"| all | 52 | {tot['ms_d']:.2f} | {tot['gf_d'] / tot['ms_d']:.1f} | {tot['gf_d'] / tot['ms_d'] / PEAK_TF:.3f} | {tot['mi_d']:.2f} | 53 | "
                 f"{tot['ms_w']:.2f} | {tot['gf_w'] / tot['ms_w']:.1f} | {tot['gf_w'] / tot['ms_w'] / PEAK_TF:.3f} | {tot['mi_w']:.2f} |")
    lines += ["", "Per launch:", "", "| # | class | Cin | Cout | out T,H,W | dgrad ms | dgrad TFLOP/s | wgrad ms | wgrad TFLOP/s | MIOpen dgrad ms | "
              "MIOpen wgrad ms |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append("| " + " | ".join(str(v) if not isinstance(v, float) else f"{v:.3f}" for v in r) + " |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="4,16,64")
    ap.add_argument("--table-batch", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-miopen", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = [f"R3D-50 trunk training, {torch.cuda.get_device_name(0)}", "",
             "| clips | forward, frozen trunk (ms) | repack alone (ms) | forward + tape + backward (ms) | ratio to the forward | train-step clips/s |",
             "|---|---|---|---|---|---|"]
    frozen = loaded(pkg.Resnet3D(app_cfg())).train(False)
    frozen.resnet.requires_grad_(False)
    m = loaded(pkg.Resnet3D(app_cfg(train_trunk=True))).train(True)
    ws = [c.weight for c in m.resnet.modules() if isinstance(c, torch.nn.Conv3d)]
    lib = pkg._lib.load()
    for B in [int(b) for b in a.batches.split(",")]:
        video = pkg.synth.make_video(B, seed=1).to(DEV)
        with torch.no_grad():
            t_fwd = BR.time_events(lambda: frozen.forward_features({"video_frames": video}), a.warmup, a.reps)
            m.forward_features({"video_frames": video})  # makes the copies once
        runner = m._runner
        _, fwd, dgr = runner.copies
        p = pkg._lib.R3dParams()
        p.bn_eps = 1e-5
        for i, (conv, bn) in enumerate(R3D.trunk_convs(m.resnet)):
            p.conv[i] = pkg._lib.R3dConv(fwd[i].data_ptr(), bn.weight.data_ptr(), bn.bias.data_ptr(), bn.running_mean.data_ptr(), bn.running_var.data_ptr())
        wp = pkg._lib.R3dPointers(*[w.data_ptr() for w in ws])
        fp, dp = pkg._lib.R3dPointers(*[t.data_ptr() for t in fwd]), pkg._lib.R3dPointers(*[t.data_ptr() for t in dgr])
        st = torch.cuda.current_stream().cuda_stream
        t_rep = BR.time_events(lambda: pkg._lib.check(lib.stlt_r3d_repack_all(wp, ctypes.byref(p), fp, dp, st), "repack_all"), a.warmup, a.reps)

        def step():
            f = m.forward_features({"video_frames": video})
            torch.autograd.grad(f, ws, torch.ones_like(f))
        t_tr = BR.time_events(step, a.warmup, a.reps)
        lines.append(f"| {B} | {t_fwd:.2f} | {t_rep:.2f} | {t_tr:.2f} | {t_tr / t_fwd:.2f} | {B / t_tr * 1e3:.0f} |")
        print(lines[-1], flush=True)
        del video
        torch.cuda.empty_cache()
    del frozen, m
    lines += ["", "| model | clips | Trainer.step (ms) | clips/s |", "|---|---|---|---|"]
    k = pkg.synth.model_kwargs("cfg1")
    for name, B in (("resnet3d", 16), ("resnet3d", 64), ("cacnf", 16)):
        if name == "resnet3d":
            model, batch = loaded(pkg.Resnet3D(app_cfg(train_trunk=True))), {}
        else:
            cfg = pkg.MultimodalModelConfig(**dict(k, appearance_num_frames=32, appearance_trunk=True, train_trunk=True))
            model = loaded(pkg.CrossAttentionCentralNetFusion(cfg))
            c = pkg.synth.CONFIGS["cfg1"]
            batch = {kk: v.to(DEV) for kk, v in pkg.synth.make_batch(B, c["T"], c["N"], seed=3).items()}
        batch["video_frames"] = pkg.synth.make_video(B, seed=2).to(DEV)
        batch["labels"] = torch.randint(0, k["num_classes"], (B,), generator=torch.Generator().manual_seed(0)).to(DEV)
        tr = pkg.train.Trainer(model, "something", learning_rate=5e-5, warmup_steps=0, total_steps=1000)
        t = BR.time_events(lambda: tr.step(batch), a.warmup, a.reps)
        lines.append(f"| {name} | {B} | {t:.1f} | {B / t * 1e3:.0f} |")
        print(lines[-1], flush=True)
        del model, tr, batch
        torch.cuda.empty_cache()
    trunk_table(a, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
