"""Dev probe (GPU box): sha256 of everything one encoder training step produces -- the cost map, every parameter gradient, every
BatchNorm buffer -- for each case of tests/test_encoder_train_launches_gpu.py, from fixed seeds.  Two trees whose files are equal
compute the same bits on this path (fixed-order partial sums everywhere): run it on both and compare.
Usage: python tools/probe_encoder_train_bits.py OUT.json          (write the digests)
       python tools/probe_encoder_train_bits.py --compare A.json B.json [...]   (exit 1 and name the tensors if any file differs from A)"""
import hashlib
import json
import os
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "neural-astar_amd"), ROOT, os.path.join(ROOT, "tests")]
import test_encoder_train_launches_gpu as T  # noqa: E402


def _sha(t):
    t = t.detach().cpu().contiguous()
    return hashlib.sha256(str((t.dtype, tuple(t.shape))).encode() + t.view(torch.uint8).numpy().tobytes()).hexdigest()


def digests(name, na, cost, launches=None):
    out = {"cost": _sha(cost)}
    for k, p in na.encoder.named_parameters():
        out["grad/" + k] = _sha(p.grad) if p.grad is not None else None
    for k, b in na.encoder.named_buffers():
        out["buffer/" + k] = _sha(b.reshape(1) if b.dim() == 0 else b)
    return out


def compare(paths):
    runs = [json.load(open(p)) for p in paths]
    bad = [(p, case, k) for p, r in zip(paths[1:], runs[1:]) for case in runs[0] for k in runs[0][case]
           if r.get(case, {}).get(k) != runs[0][case][k]]
    bad += [(p, case, "<missing in the first file>") for p, r in zip(paths[1:], runs[1:]) for case in r if case not in runs[0]]
    n = sum(len(v) for v in runs[0].values())
    print(json.dumps({"files": paths, "cases": len(runs[0]), "tensors": n, "different": bad}))
    return 1 if bad else 0


def main():
    if sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2:]))
    import torch.multiprocessing as mp
    dev = torch.device("cuda:0")
    res = {}
    for name, case in T.CASES.items():
        if not case[7]:
            res[name] = digests(name, *T.run_case(name, dev))
    with tempfile.TemporaryDirectory() as tmp:  # the sync cases need a process group: a child of their own, as in the test
        mp.spawn(T.sync_worker, args=(T.free_port(), tmp, [n for n, c in T.CASES.items() if c[7]], digests), nprocs=1, join=True)
        res.update(json.load(open(os.path.join(tmp, "sync.json"))))
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    json.dump(res, open(sys.argv[1], "w"), indent=1, sort_keys=True)
    print(f"{len(res)} cases, {sum(len(v) for v in res.values())} tensors -> {sys.argv[1]}")


if __name__ == "__main__":
    main()
