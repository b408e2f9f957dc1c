#!/usr/bin/env python3
"""What the log-policy costs on the TILED soft field (include/nastar_soft_policy_tiled.h): on 4 random maps of 512x512 (25 % obstacles, costs
U(0.1, 1), Moore-8, tau = 0.25) at the default horizon 2 * (H + W) = 2048 and the default checkpoint spacing ceil(sqrt(K)),

  forward   ``nastar_soft_policy_forward_tiled`` against ``nastar_soft_cost_to_go_tiled`` with the policy, both without a tape and with one;
  backward  ``nastar_soft_policy_backward_tiled`` with GL alone, with G and GL, and with G alone, against
            ``nastar_soft_fields_backward_tiled``.

The sibling of tools/probe_soft_fields_tiled.py, with its method: device events around ONE call (all its launches), after warm-up; here
the variants of one repetition run back to back, so a drift of the machine reaches all of them alike, and each figure is the median / min /
max over the repetitions.  The measuring runs in a CHILD process with a time limit of its own.  ``--baseline-lib`` names another build of
the C ABI (the parent commit's, say): a second child times the field calls of THAT library (``NASTAR_LIB``), and the two children are run
alternately ``--rounds`` times, so the field calls of both builds are measured in the same visit.  A probe, not a gate: there is no
target.  Writes one JSON document.

Usage:  python tools/probe_soft_policy_tiled.py [--reps 10] [--rounds 2] [--baseline-lib PATH] [--out profiles/soft_policy_tiled.json] [--small]
"""
import argparse
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOORE8 = 0x1EF
TAU = 0.25


def child(args):
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, "neural-astar_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import soft_fields_oracle as SO
    from neural_astar import _native

    dev = torch.device("cuda:0")
    lib = _native.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    B, H, W = (1, 96, 136) if args.small else (4, 512, 512)
    K = 2 * (H + W)
    ck = math.isqrt(K - 1) + 1
    cost, passable, goal = SO.random_maps(H * W, B, H, W)
    rng = np.random.default_rng(1)
    c, p, g = (torch.from_numpy(a).to(dev) for a in (cost, passable, goal))
    G = torch.from_numpy(rng.standard_normal((B, H, W)).astype(np.float32)).to(dev)
    GL = torch.from_numpy(rng.standard_normal((B, 8, H, W)).astype(np.float32)).to(dev)
    dist, grad = torch.empty_like(c), torch.empty_like(c)
    pol, logp = torch.empty((B, 8, H, W), dtype=torch.float32, device=dev), torch.empty((B, 8, H, W), dtype=torch.float32, device=dev)
    st = torch.zeros((B,), dtype=torch.int32, device=dev)
    ws = torch.empty((int(lib.nastar_soft_fields_tiled_workspace_bytes(B, H, W)),), dtype=torch.uint8, device=dev)
    tape = torch.empty((int(lib.nastar_soft_fields_tiled_tape_bytes(B, H, W, K, ck)),), dtype=torch.uint8, device=dev)
    bws = torch.empty((int(lib.nastar_soft_fields_tiled_backward_workspace_bytes(B, H, W, K, ck)),), dtype=torch.uint8, device=dev)
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731

    def field_forward(with_tape):
        _native.check(lib.nastar_soft_cost_to_go_tiled(ptr(c), ptr(g), ptr(p), B, H, W, MOORE8, TAU, K, ptr(dist), ptr(pol), ptr(st),
                                                       ptr(tape) if with_tape else None, tape.numel() if with_tape else 0, ck, ptr(ws), ws.numel(),
                                                       stream), "nastar_soft_cost_to_go_tiled")

    def policy_forward(with_tape):
        _native.check(lib.nastar_soft_policy_forward_tiled(ptr(c), ptr(g), ptr(p), B, H, W, MOORE8, TAU, K, ptr(dist), ptr(pol), ptr(logp), ptr(st),
                                                           ptr(tape) if with_tape else None, tape.numel() if with_tape else 0, ck, ptr(ws),
                                                           ws.numel(), stream), "nastar_soft_policy_forward_tiled")

    def field_backward():
        _native.check(lib.nastar_soft_fields_backward_tiled(ptr(c), ptr(g), ptr(p), ptr(tape), tape.numel(), ck, ptr(G), B, H, W, MOORE8, TAU, K,
                                                            ptr(grad), ptr(st), ptr(bws), bws.numel(), stream), "nastar_soft_fields_backward_tiled")

    def policy_backward(up, upl):
        _native.check(lib.nastar_soft_policy_backward_tiled(ptr(c), ptr(g), ptr(p), ptr(tape), tape.numel(), ck, ptr(up), ptr(upl), B, H, W, MOORE8,
                                                            TAU, K, ptr(grad), ptr(st), ptr(bws), bws.numel(), stream),
                      "nastar_soft_policy_backward_tiled")

    variants = {"field_forward": lambda: field_forward(False), "field_forward_tape": lambda: field_forward(True), "field_backward": field_backward}
    if not args.fields_only:
        assert int(lib.nastar_soft_policy_tiled_backward_workspace_bytes(B, H, W, K, ck)) == bws.numel()
        variants.update({"policy_forward": lambda: policy_forward(False), "policy_forward_tape": lambda: policy_forward(True),
                         "policy_backward_GL": lambda: policy_backward(None, GL), "policy_backward_G_GL": lambda: policy_backward(G, GL),
                         "policy_backward_G": lambda: policy_backward(G, None)})
    field_forward(True)                                             # the tape every backward reads
    for _ in range(2):                                              # warm-up: every variant, every shape it uses
        for launch in variants.values():
            launch()
    torch.cuda.synchronize()
    ms = {name: [] for name in variants}
    for _ in range(args.reps):
        for name, launch in variants.items():                       # back to back: one repetition of every variant, then the next
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            launch()
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b))
    assert st.tolist() == [0] * B and bool(torch.isfinite(grad).all())
    props = torch.cuda.get_device_properties(dev)
    row = {"library": os.path.relpath(_native.LIB_PATH, ROOT), "B": B, "H": H, "W": W, "horizon": K, "checkpoint_every": ck, "tau": TAU,
           "neighbor_mask": MOORE8, "reps": args.reps, "tape_bytes": tape.numel(), "backward_workspace_bytes": bws.numel(),
           "ms": {n: {"median": float(np.median(t)), "min": float(np.min(t)), "max": float(np.max(t))} for n, t in ms.items()},
           "device": torch.cuda.get_device_name(dev), "compute_units": props.multi_processor_count,
           "timing": "device events around one call (all its launches), after 2 warm-up calls; the variants of a repetition back to back"}
    print("PROBE " + json.dumps(row), flush=True)


def run_child(args, baseline):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps)] + (["--small"] if args.small else [])
    env = dict(os.environ)
    if baseline:
        cmd.append("--fields-only")
        env["NASTAR_LIB"] = os.path.abspath(args.baseline_lib)
    done = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, timeout=args.timeout)   # (a child past its limit is killed)
    if done.returncode != 0:
        raise SystemExit(f"the measuring child failed with status {done.returncode}; nothing more is started")
    return json.loads(next(line for line in done.stdout.splitlines() if line.startswith("PROBE "))[len("PROBE "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2, help="how often the children are run (alternately, with --baseline-lib)")
    ap.add_argument("--baseline-lib", default=None, help="another build of the C ABI whose field calls are timed beside this one's")
    ap.add_argument("--timeout", type=float, default=240.0, help="seconds a measuring child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "soft_policy_tiled.json"))
    ap.add_argument("--small", action="store_true", help="one 96x136 map (a rehearsal)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--fields-only", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    runs = []
    for r in range(args.rounds):
        runs.append(dict(run_child(args, False), build="this", round=r))
        if args.baseline_lib:
            runs.append(dict(run_child(args, True), build="baseline", round=r))
    med = lambda build, name: [run["ms"][name]["median"] for run in runs if run["build"] == build and name in run["ms"]]  # noqa: E731
    mid = lambda xs: sorted(xs)[len(xs) // 2] if xs else None  # noqa: E731
    this = {n: mid(med("this", n)) for n in runs[0]["ms"]}
    summary = {"median_ms": this,
               "forward_logp_over_field": this["policy_forward"] / this["field_forward"],
               "forward_tape_logp_over_field": this["policy_forward_tape"] / this["field_forward_tape"],
               "backward_GL_over_field": this["policy_backward_GL"] / this["field_backward"],
               "backward_G_GL_over_field": this["policy_backward_G_GL"] / this["field_backward"],
               "backward_G_over_field": this["policy_backward_G"] / this["field_backward"]}
    if args.baseline_lib:
        base = {n: mid(med("baseline", n)) for n in ("field_forward", "field_forward_tape", "field_backward")}
        summary.update(baseline_median_ms=base, field_calls_this_over_baseline={n: this[n] / base[n] for n in base})
    doc = {"probe": "tools/probe_soft_policy_tiled.py", "summary": summary, "runs": runs}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(summary, indent=1))


if __name__ == "__main__":
    main()
