"""Same-numbers check for a refactor: does a branch compute what its parent computed?

``dump`` (run once per checkout, twice in the parent's) records, with fixed seeds, every output, input
gradient and parameter gradient of one forward + backward of six ResNet bottleneck blocks (bf16 NHWC, batch 2:
the blocks of ``tests/test_resnet_routing_gpu.py``) and the logits, losses, parameter gradients and final
parameters of two resnet50 training steps (batch 4, 64x64, DP wrapper + FusedSGD).  ``compare`` takes two dumps
of the parent and one of the branch: a tensor that is ``torch.equal`` between the two parent runs must be
``torch.equal`` between parent and branch; one that does not reproduce on the parent itself (the library's
weight gradients) is compared by relative norm, and the branch may be at most twice as far from a parent run as
the two parent runs are from each other (the spread is a single sample, hence the factor).  More dumps per
side sample that spread better: a tensor is then held bitwise only if every parent run agrees on it, the
spread is the largest parent-parent distance, and every branch run is measured to its nearest parent run.

    python bench/refactor_equiv.py dump parent_a.pt         # in the parent's checkout, twice (a, b)
    python bench/refactor_equiv.py dump branch.pt           # in the branch's checkout
    python bench/refactor_equiv.py compare --parent parent_a.pt parent_b.pt --branch branch.pt --out report.json

``MADNN_WGRAD=k12 MADNN_K9_WGRAD=k9 MADNN_CONV3X3_WGRAD=k13`` pins the weight gradients to madnn's own
(deterministic) kernels, which leaves few tensors to the relative-norm rule.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.getcwd())   # the checkout the command is run in, not the one holding this file


def _blocks():
    import madnn.models.resnet as R

    def ds(cin, cout, stride=1):
        return torch.nn.Sequential(R.conv1x1(cin, cout, stride), R.BN(cout))

    return {
        "identity_64": (lambda: R.Bottleneck(256, 64), 256, 8),
        "downsample_s1_64": (lambda: R.Bottleneck(64, 64, downsample=ds(64, 256)), 64, 8),
        "identity_128": (lambda: R.Bottleneck(512, 128), 512, 8),
        "downsample_s2_128": (lambda: R.Bottleneck(256, 128, stride=2, downsample=ds(256, 512, 2)), 256, 8),
        "downsample_s2_512": (lambda: R.Bottleneck(1024, 512, stride=2, downsample=ds(1024, 2048, 2)), 1024, 8),
        "identity_512": (lambda: R.Bottleneck(2048, 512), 2048, 4),
    }


def dump(path):
    import madnn
    from madnn.models import resnet50
    from madnn.optim import FusedSGD

    assert madnn.ops.load_kernels()
    dev = torch.device("cuda", 0)
    out = {}
    for name, (make, cin, hw) in _blocks().items():
        torch.manual_seed(1)
        blk = make()
        for m in blk.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                torch.nn.init.uniform_(m.weight, 0.5, 1.5)
                torch.nn.init.normal_(m.bias, 0, 0.2)
        blk = blk.to(dev).to(memory_format=torch.channels_last).train()
        for p in blk.parameters():
            if p.dim() == 4:
                p.data = p.data.bfloat16().contiguous(memory_format=torch.channels_last)
        g = torch.Generator(device=dev).manual_seed(2)
        x = torch.randn(2, cin, hw, hw, device=dev, generator=g).bfloat16().contiguous(memory_format=torch.channels_last)
        x.requires_grad_(True)
        y = blk(x)
        y.backward(torch.randn(y.shape, device=dev, generator=g).bfloat16().contiguous(memory_format=torch.channels_last))
        out[f"{name}/out"], out[f"{name}/x.grad"] = y.detach(), x.grad
        for k, p in blk.named_parameters():
            out[f"{name}/{k}.grad"] = p.grad
        for k, b in blk.named_buffers():
            out[f"{name}/{k}"] = b.detach().clone()
    torch.manual_seed(0)
    model = resnet50(num_classes=100)
    opt = FusedSGD(model.parameters(), lr=0.05, momentum=0.9)
    dmodel, opt = madnn.distribute(model, opt, strategy="dp")
    x, y = madnn.data.synthetic_batch("image", 4, dev, channels_last=True, num_classes=100, shape=(3, 64, 64))
    for step in range(2):
        logits = dmodel(x)
        loss = F.cross_entropy(logits.float(), y)
        loss.backward()
        out[f"resnet50/step{step}/logits"], out[f"resnet50/step{step}/loss"] = logits.detach().clone(), loss.detach().clone()
        for k, p in model.named_parameters():
            if p.grad is not None:
                out[f"resnet50/step{step}/{k}.grad"] = p.grad.detach().clone()
        opt.step()
    for k, p in model.named_parameters():
        out[f"resnet50/final/{k}"] = p.detach().clone()
    torch.cuda.synchronize()
    torch.save({k: v.cpu() for k, v in out.items()}, path)
    print(f"{len(out)} tensors -> {path}; per-shape timings run: {madnn.ops.tuning_timings()}")


def _dist(a, b):
    den = a.double().norm().item()
    num = (a.double() - b.double()).norm().item()
    return num if den == 0.0 else num / den


def compare(parents, branches, report):
    pa, br = [torch.load(p) for p in parents], [torch.load(p) for p in branches]
    assert all(d.keys() == pa[0].keys() for d in pa + br), "the dumps hold different tensors"
    bad, loose = [], {}
    for k, ref in pa[0].items():
        if all(torch.equal(ref, d[k]) for d in pa[1:]):
            if not all(torch.equal(ref, d[k]) for d in br):
                bad.append({"tensor": k, "rule": "bitwise", "branch_vs_parent": max(_dist(ref, d[k]) for d in br)})
        else:
            spread = max(_dist(a[k], b[k]) for i, a in enumerate(pa) for b in pa[i + 1:])
            dist = max(min(_dist(a[k], d[k]) for a in pa) for d in br)   # each branch run to its nearest parent run
            loose[k] = {"parent_vs_parent": spread, "branch_vs_parent": dist}
            if not dist <= 2.0 * spread:
                bad.append({"tensor": k, "rule": "2x parent spread", **loose[k]})
    res = {"parent_runs": len(pa), "branch_runs": len(br), "tensors": len(pa[0]),
           "bitwise_reproducible_on_parent": len(pa[0]) - len(loose), "relative_norm": loose, "failed": bad}
    print(json.dumps({**res, "relative_norm": f"{len(loose)} tensors"}, indent=1))
    for k, v in loose.items():
        print(f"  not reproducible on the parent: {k}: parent-parent {v['parent_vs_parent']:.3e} "
              f"branch-parent {v['branch_vs_parent']:.3e}")
    if report:
        with open(report, "w") as f:
            json.dump(res, f, indent=1)
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    sub.add_parser("dump").add_argument("path")
    cp = sub.add_parser("compare")
    cp.add_argument("--parent", nargs="+", required=True, help="two or more dumps of the parent")
    cp.add_argument("--branch", nargs="+", required=True, help="one or more dumps of the branch")
    cp.add_argument("--out")
    args = ap.parse_args()
    sys.exit(dump(args.path) if args.cmd == "dump" else compare(args.parent, args.branch, args.out))
