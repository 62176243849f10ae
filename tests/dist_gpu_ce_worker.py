"""Worker for tests/test_gpu_supervised.py: one native supervised (cross-entropy) step on cuda:0
as rank RANK of WORLD_SIZE (gloo carries the collectives, so the ranks share the one GPU of the
test box). Writes the gradient the optimizer applies (flat gradient x grad_scale) to OUT_DIR."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main():
    out_dir = sys.argv[1]
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    from simclr_pytorch_distributed_amd.config import parse_ce
    from simclr_pytorch_distributed_amd.engine.supervised import SupervisedEngine
    from simclr_pytorch_distributed_amd.models.executor import to_nhwc_input
    from simclr_pytorch_distributed_amd.models.resnet import SupCEResNet
    from simclr_pytorch_distributed_amd.ops.ce_head import classifier_ce
    G = 32                                                     # global images
    argv = ["--model", "resnet18", "--backend", "native", "--dist_backend", "gloo", "--synthetic",
            "--synthetic_size", "64", "--learning_rate", "0.05", "--work_dir", out_dir, "--batch_size", str(G),
            "--ngpu", str(world)]
    if world > 1:
        argv += ["--syncBN", "--syncbn_comm", "rccl"]          # over gloo: the Python collective path
    opt = parse_ce(argv, make_dirs=False)
    eng = SupervisedEngine(opt, device=torch.device("cuda:0"))
    torch.manual_seed(123)
    eng.model.load_state_dict(SupCEResNet("resnet18", 10).state_dict())
    eng.model.train()
    g = torch.Generator().manual_seed(7)
    imgs = torch.randn(G, 3, 32, 32, generator=g)
    labels = torch.randint(0, 10, (G,), generator=g)
    per = G // world
    sl = slice(rank * per, (rank + 1) * per)
    feat = eng.runner.encode(to_nhwc_input(imgs[sl].cuda()))
    loss, stats = classifier_ce(feat, eng.model.fc, labels[sl].cuda())
    eng.optimizer.zero_grad()
    loss.backward()
    if eng.reducer is not None:
        eng.reducer.finish()
    grad = (eng.flat.grad.detach() * eng.optimizer.grad_scale).clone()
    eng.optimizer.step()
    torch.cuda.synchronize()
    torch.save({"grad": grad.cpu(), "flat": eng.flat.flat.detach().cpu(), "loss": float(loss.detach()),
                "stats": stats.cpu(), "names": list(eng.flat.names), "offsets": [int(o) for o in eng.flat.offsets],
                "numels": [p.numel() for p in eng.flat.params]}, os.path.join(out_dir, f"ce_w{world}_r{rank}.pt"))
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
