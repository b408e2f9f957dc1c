#!/usr/bin/env python3
"""Randomised parity sweep (run on the GPU box): the search through the C ABI against the oracle's state-machine restatement on random map
sizes (LDS-resident, compiled and hand-scheduled instantiations, and the hybrid large-map kernel just above the LDS limit), obstacle
densities, cost kinds (map / U(0,1) / U(0,10)), g_ratio and budgets, with and without a selection log and a random placement.  Prints one
JSON line per failing case and a summary; exit code 1 on any mismatch."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "neural-astar_amd"), ROOT]
sys.path.append(os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from neural_astar import ops  # noqa: E402
from neural_astar.utils import synthetic as syn  # noqa: E402
from oracle import oracle as O  # noqa: E402

dev = torch.device("cuda:0")
sizes = [(16, 16), (32, 32), (64, 64), (12, 12), (7, 5), (20, 45), (64, 128), (100, 100), (128, 128), (130, 131), (135, 150), (140, 140), (150, 200), (33, 31),
         (96, 96), (48, 80), (5, 200), (200, 5), (1, 40), (40, 1), (129, 129), (131, 127)]


def run(seed=20260926, N=160, big_frac=0.15, verbose=True):
  """-> (cases per kernel family, list of failing case descriptions)"""
  rng = np.random.default_rng(seed)
  bad = []
  stats = {}
  for case in range(N):
    if case < 2 * len(sizes):
        H, W = sizes[case % len(sizes)]
    elif rng.random() < big_frac:  # above the LDS limit: the hybrid kernel (fill / search / store launches)
        H, W = int(rng.integers(120, 260)), int(rng.integers(120, 260))
    elif rng.random() < 0.3:       # the hand-scheduled instruction streams (general and unit-cost layouts)
        H = W = int(rng.choice([16, 32, 64]))
    else:
        H, W = int(rng.integers(3, 160)), int(rng.integers(3, 160))
    B = int(rng.integers(1, 9))
    p = float(rng.choice([0.0, 0.1, 0.2, 0.3]))
    try:
        pr = syn.random_obstacle_maps(B, H, W, p, seed=int(rng.integers(1 << 30)))
    except Exception:
        continue
    kind = str(rng.choice(["map", "u01", "u10", "signed", "zeros"]))
    if kind == "map":
        cost = pr.map_designs
    elif kind == "signed":  # negative costs: the round-2 instruction stream with its order-preserving key transform (16 / 32 / 64), generic paths elsewhere
        cost = syn.random_costs(B, H, W, seed=int(rng.integers(1 << 30)), lo=-0.5, hi=1.0)
    elif kind == "zeros":   # many exactly-zero costs: ties in g as well as in h
        cost = syn.random_costs(B, H, W, seed=int(rng.integers(1 << 30))) * (rng.random((B, 1, H, W)) < 0.5).astype(np.float32)
    else:
        cost = syn.random_costs(B, H, W, seed=int(rng.integers(1 << 30)), hi=1.0 if kind == "u01" else 10.0)
    maps = pr.map_designs.copy()
    starts = pr.start_maps
    variant = str(rng.choice(["plain", "plain", "plain", "start_on_obstacle", "start_is_goal"]))
    if variant == "start_on_obstacle":  # the start is expanded even on an obstacle (reference :187: open = start)
        maps.reshape(B, -1)[np.arange(B), pr.start_maps.reshape(B, -1).argmax(1)] = 0.0
        if kind == "map":
            cost = maps
    elif variant == "start_is_goal":
        starts = pr.goal_maps.copy()
    pr = syn.Problems(maps, starts, pr.goal_maps)
    unit = kind == "map" and H == W and W in (32, 64) and rng.random() < 0.5  # the unit-cost LDS layout (NASTAR_FLAG_UNIT_COST)
    gr = float(rng.choice([0.5, 0.5, 0.5, 0.2, 0.8, 0.0, 1.0]))
    T = W * W if rng.random() < 0.7 else max(1, int(rng.choice([0.05, 0.25, 0.5]) * W * W))
    log = bool(rng.random() < 0.5) and not unit
    in_lds = ops.in_lds(H, W)
    order = None
    if in_lds and rng.random() < 0.4:
        order = torch.from_numpy(rng.permutation(B).astype(np.int32)).to(dev)
    c, s, g, m = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (cost, pr.start_maps, pr.goal_maps, pr.map_designs))
    try:
        hist, paths, iters, status, sel = ops.search_nograd(c, s, g, c if kind == "map" else m, gr, T, want_log=log, order=order, check_order=False,
                                                            flags=ops.FLAG_UNIT_COST if unit else 0)
        torch.cuda.synchronize()
        o = O.forward(cost, pr.start_maps, pr.goal_maps, pr.map_designs, gr, T, mode="sm", want_log=log)
        ok = (np.array_equal(hist.cpu().numpy(), o.histories) and np.array_equal(paths.cpu().numpy(), o.paths) and np.array_equal(iters.cpu().numpy(), o.iters)
              and bool((status == 0).all()))
        if ok and log:
            lg, it = sel.cpu().numpy(), o.iters
            ok = all(np.array_equal(lg[b, :it[b]], o.sel_log[b, :it[b]]) for b in range(B))
    except Exception as e:  # noqa: BLE001
        ok = False
        if verbose:
            print(json.dumps({"case": case, "error": f"{type(e).__name__}: {e}"[:300]}), flush=True)
    key = ("unit" if unit else "lds") if in_lds else "hybrid"
    stats[key] = stats.get(key, 0) + 1
    if not ok:
        d = {"case": case, "H": H, "W": W, "B": B, "p": p, "cost": kind, "variant": variant, "unit": bool(unit), "g_ratio": gr, "max_iters": T, "log": log,
             "placed": order is not None, "in_lds": in_lds}
        bad.append(d)
        if verbose:
            print(json.dumps(d), flush=True)
  return stats, bad


def run_backward(seed=11, N=40, verbose=True, large=False):
    """dL/dcost of the replay backward (through DifferentiableAstar under autograd) against the oracle's literal reverse-mode restatement on
    random small maps (``large``: 64 .. 140 cells per side -- the generic LDS replay and the one with its state in the HBM workspace; the
    oracle needs seconds per map there), training and eval budgets, random upstream gradients; tolerance 1e-5 (north_star).
    -> (cases, failures)"""
    from neural_astar.planner.differentiable_astar import DifferentiableAstar
    rng = np.random.default_rng(seed)
    small = [(16, 16), (32, 32), (12, 12), (7, 5), (20, 45), (33, 31), (24, 40), (48, 48), (9, 30)]
    if large:
        small = [(64, 64), (96, 96), (100, 100), (110, 130), (140, 90), (128, 128)]
    bad, n = [], 0
    for case in range(N):
        H, W = small[case % len(small)] if (large or case < 2 * len(small)) else (int(rng.integers(4, 50)), int(rng.integers(4, 50)))
        B = int(rng.integers(1, 3 if large else 5))
        pr = syn.random_obstacle_maps(B, H, W, float(rng.choice([0.0, 0.15, 0.3])), seed=int(rng.integers(1 << 30)))
        cost_np = syn.random_costs(B, H, W, seed=int(rng.integers(1 << 30)))
        gr = float(rng.choice([0.5, 0.5, 0.2, 0.8]))
        train = bool(rng.random() < 0.5)
        Tmax = float(rng.choice([0.05, 0.1] if large else [0.25, 0.5, 1.0])) if train else 1.0
        T = int((Tmax if train else 1.0) * W * W)
        if T < 1:
            continue
        up = rng.standard_normal((B, 1, H, W)).astype(np.float32)
        da = DifferentiableAstar(gr, Tmax).to(dev).train(train)
        cost = torch.from_numpy(cost_np).to(dev).requires_grad_(True)
        s, g, m = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (pr.start_maps, pr.goal_maps, pr.map_designs))
        out = da(cost, s, g, m)
        (out.histories * torch.from_numpy(up).to(dev)).sum().backward()
        ref = O.backward(up, cost_np, pr.start_maps, pr.goal_maps, pr.map_designs, gr, T)
        err = float(np.abs(cost.grad[:, 0].cpu().numpy() - ref).max())
        n += 1
        if not err <= 1e-5 * max(1.0, float(np.abs(ref).max())):
            d = {"case": case, "H": H, "W": W, "B": B, "g_ratio": gr, "train": train, "Tmax": Tmax, "err": err}
            bad.append(d)
            if verbose:
                print(json.dumps(d), flush=True)
    return n, bad


def run_module(seed=31, N=60, verbose=True, grad_frac=0.35, large_frac=0.1, large_hw=((112, 151), (112, 201))):
    """DifferentiableAstar.forward() against the oracle's LITERAL restatement of the reference's batch loop, on random batches incl. the cost
    kinds / g_ratio values of the batch-coupled class.  Round 6: every mode -- same-call verdict, deferred (verdict
    collected before the outputs are read), unchecked (where the class is reachable with costs >= 0 the exact pipeline runs anyway) --, a share
    of the cases UNDER AUTOGRAD (dL/dcost against the oracle's literal reverse mode, 1e-5) and a share on maps whose state does not fit LDS
    (the hybrid kernel's lock-step modes; up to 150x200 -- the oracle's dense restatement needs tens of seconds for one of those).
    -> (cases, batches in the coupled class, gradient cases, failures)"""
    import warnings
    from neural_astar.planner.differentiable_astar import DifferentiableAstar
    rng = np.random.default_rng(seed)
    bad, n, reruns, ngrad = [], 0, 0, 0
    for case in range(N):
        large = rng.random() < large_frac
        if large:
            H, W = int(rng.integers(*large_hw[0])), int(rng.integers(*large_hw[1]))
        else:
            H, W = (int(rng.integers(4, 40)), int(rng.integers(4, 40))) if rng.random() < 0.8 else (int(rng.choice([16, 32])),) * 2
        B = int(rng.integers(2, 4 if large else 6))
        pr = syn.random_obstacle_maps(B, H, W, float(rng.choice([0.0, 0.1, 0.25])), seed=int(rng.integers(1 << 30)))
        kind = str(rng.choice(["map", "u01", "u10", "u10", "zeros", "signed", "signed2"]))
        if kind == "map":
            cost = pr.map_designs
        elif kind == "zeros":
            cost = syn.random_costs(B, H, W, seed=int(rng.integers(1 << 30))) * (rng.random((B, 1, H, W)) < 0.5).astype(np.float32)
        elif kind == "signed":  # negative costs (the 16 / 32 / 64 streams take the key transform)
            cost = syn.random_costs(B, H, W, seed=int(rng.integers(1 << 30)), lo=-0.5, hi=1.0)
        elif kind == "signed2":  # costs below -1: the batch-coupled class at ANY g_ratio (found through the status summary for g_ratio in [0.5, 1))
            cost = syn.random_costs(B, H, W, seed=int(rng.integers(1 << 30)), lo=-2.0, hi=1.0)
        else:
            cost = syn.random_costs(B, H, W, seed=int(rng.integers(1 << 30)), hi=1.0 if kind == "u01" else 10.0)
        gr = float(rng.choice([0.5, 0.2, 0.0, 0.8, 1.0, 0.3]))
        train = bool(rng.random() < 0.3)
        Tmax = float(rng.choice([0.25, 0.5])) if train else 1.0
        T = int(Tmax * W * W) if train else W * W
        if T < 1:
            continue
        o = O.forward(cost, pr.start_maps, pr.goal_maps, pr.map_designs, gr, T, mode="dense")
        if o.status:
            continue  # (negative costs can empty an open list: the reference crashes there)
        osm = O.forward(cost, pr.start_maps, pr.goal_maps, pr.map_designs, gr, T, mode="sm")
        reruns += int(not np.array_equal(o.histories, osm.histories))
        with_grad = kind != "map" and rng.random() < grad_frac and H * W <= 32000
        mode = [True, "deferred", False][int(rng.integers(0, 3))]
        if mode is False and not ops.coupling_possible(gr):
            mode = True  # (the documented gap: unchecked calls read nothing back, and only costs below -1 reach the class at this g_ratio)
        if mode == "deferred" and with_grad and not ops.coupling_possible(gr):
            mode = True  # (deferred + autograd + costs below -1: refused loudly by design)
        da = DifferentiableAstar(gr, Tmax, check_solvable=mode).to(dev).train(train)
        c, s, g, m = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (cost, pr.start_maps, pr.goal_maps, pr.map_designs))
        err = None
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("error")
                if with_grad:
                    up = rng.standard_normal((B, 1, H, W)).astype(np.float32)
                    cg = c.clone().requires_grad_(True)
                    out = da(cg, s, g, m)
                    (out.histories * torch.from_numpy(up).to(dev)).sum().backward()
                    da.raise_if_unsolvable()
                    ref = O.backward(up, cost, pr.start_maps, pr.goal_maps, pr.map_designs, gr, T)
                    gerr = float(np.abs(cg.grad[:, 0].cpu().numpy() - ref).max())
                    ngrad += 1
                    if not gerr <= 1e-5 * max(1.0, float(np.abs(ref).max())):
                        err = f"grad err {gerr:.3e} (scale {float(np.abs(ref).max()):.3e})"
                else:
                    with torch.no_grad():
                        out = da(c, s, g, c if kind == "map" else m)
                        da.raise_if_unsolvable()
            ok = np.array_equal(out.histories[:, 0].detach().cpu().numpy(), o.histories) and np.array_equal(out.paths[:, 0].cpu().numpy(), o.paths)
            if not ok:
                err = "histories / paths differ from the literal batch loop"
        except Exception as e:  # noqa: BLE001
            err = f"{type(e).__name__}: {e}"[:300]
        n += 1
        if err:
            d = {"case": case, "H": H, "W": W, "B": B, "cost": kind, "g_ratio": gr, "train": train, "Tmax": Tmax, "mode": str(mode), "grad": bool(with_grad), "error": err}
            bad.append(d)
            if verbose:
                print(json.dumps(d), flush=True)
        if verbose and case % 20 == 19:
            print(json.dumps({"module_cases_so_far": n, "of": case + 1, "coupled": reruns, "with_grad": ngrad, "failures": len(bad)}), flush=True)
    run_module.ngrad = ngrad
    return n, reruns, bad


def run_encoder(seed=21, N=30, verbose=True):
    """cost maps of the MI355X inference encoders (f16x3: the default backend) against the SAME module on torch.nn fp32, random depths / map
    sizes / inputs / const, BatchNorm statistics and weights randomised; tolerance 1e-5 (north_star) on the cost map.  -> (cases, failures)"""
    from neural_astar.planner import NeuralAstar
    rng = np.random.default_rng(seed)
    bad, n = [], 0
    routes = {}
    for case in range(N):
        arch = "CNNDownSize" if rng.random() < 0.3 else "CNN"
        depth = int(rng.integers(1, 5))
        if arch == "CNN":
            H, W = (32, 32) if rng.random() < 0.25 else (int(rng.integers(4, 100)), int(rng.integers(4, 120)))
            gh, gw = H, W
        else:
            f = 1 << depth
            gh, gw = int(rng.integers(2, 9)), int(rng.integers(2, 9))
            H, W = gh * f, gw * f
        inp = str(rng.choice(["m+", "m"])) if arch == "CNN" else "m+"
        const = None if rng.random() < 0.5 else float(rng.choice([2.0, 10.0]))
        B = int(rng.integers(1, 6))
        torch.manual_seed(int(rng.integers(1 << 30)))
        na = NeuralAstar(encoder_input=inp, encoder_arch=arch, encoder_depth=depth, const=const, learn_obstacles=(arch == "CNNDownSize")).to(dev).eval()
        with torch.no_grad():
            for mod in na.encoder.modules():  # non-trivial BatchNorm statistics
                if isinstance(mod, torch.nn.BatchNorm2d):
                    mod.running_mean.normal_(0, 0.3)
                    mod.running_var.uniform_(0.5, 2.0)
                    mod.weight.uniform_(0.5, 1.5)
                    mod.bias.normal_(0, 0.2)
            m = (torch.rand(B, 1, H, W, device=dev) > 0.2).float()
            s = torch.zeros(B, 1, gh, gw, device=dev)
            g = torch.zeros(B, 1, gh, gw, device=dev)
            s[:, 0, 0, 0] = 1
            g[:, 0, -1, -1] = 1
            na.encoder_backend = "auto"
            try:
                import warnings
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    c_hip = na.encode(m, s, g)
                route = na.last_encoder_route
                na.encoder_backend = "torch"
                c_ref = na.encode(m, s, g)
                scale = float(const or 1.0)
                err = float((c_hip - c_ref).abs().max()) / scale
                ok = err <= 1e-5 or not route.startswith("hip")
            except Exception as e:  # noqa: BLE001
                ok, err, route = False, -1.0, f"{type(e).__name__}: {e}"[:200]
        n += 1
        routes[route.split(" ")[0]] = routes.get(route.split(" ")[0], 0) + 1
        if not ok:
            d = {"case": case, "arch": arch, "depth": depth, "H": H, "W": W, "B": B, "input": inp, "const": const, "err": err, "route": route}
            bad.append(d)
            if verbose:
                print(json.dumps(d), flush=True)
    run_encoder.routes = routes
    return n, bad


# ---- the masked kernels (DifferentiableAstar.neighbor_filter: nastar_forward_ex_masked, nastar_forward_batchloop_finish_masked,
# nastar_backward_replay_ordered_masked) against the oracle's masked restatements ------------------------------------------------------------

# NASTAR_NEIGHBORS_* encoding (include/nastar.h): bit r*3+c <=> neighbor_filter cell (r, c) is 1; filter cell (a, b) opens offset (1-a, 1-b)
MOORE8 = 0x1EF
SINGLE_BIT_MASKS = [1 << k for k in range(9) if k != 4]
MOORE_MINUS_ONE_MASKS = [MOORE8 & ~(1 << k) for k in range(9) if k != 4]
VON_NEUMANN, DIAGONALS = 0x0AA, 0x145
MASKS_CENTRE_CLEAR = [m for m in range(512) if not m & 0x10]
NAMED_MASKS = SINGLE_BIT_MASKS + MOORE_MINUS_ONE_MASKS + [VON_NEUMANN, DIAGONALS]

# widths whose division by fl32(sqrt(W)) takes the FMA path (csrc/nastar_capi.hip fastdiv_verified); every other width divides in IEEE
FASTDIV_WIDTHS = {1, 2, 4, 8, 10, 12, 16, 20, 24, 28, 32, 40, 45, 48, 50, 60, 64, 96, 100, 128, 256, 512, 1024}


def offset_of(bit):
    """the step a neighbour_filter cell allows: conv2d is a cross-correlation, filter cell (a, b) opens offset (1 - a, 1 - b)"""
    return 1 - bit // 3, 1 - bit % 3


def mask_filter(mask):
    return [[(mask >> (r * 3 + c)) & 1 for c in range(3)] for r in range(3)]


def masked_route(H, W, vec4_ok=True):
    """the forward kernel nastar_forward_ex_masked launches for an H x W batch (csrc/nastar_capi.hip: forward() -> needs_global_state ->
    forward_hybrid, else forward_lds -> compact_kernel<kMasked = true>, vec4 = W % 4 == 0 with 16-byte aligned tensors, fast = fastdiv_verified(W),
    CPL = chunks of 16 cells per lane of 64 (make_cdims)).  `vec4_ok`: False for a tensor off 16-byte alignment"""
    fast = W in FASTDIV_WIDTHS
    if not ops.in_lds(H, W):
        return "hybrid_fastdiv" if fast else "hybrid_ieee"
    vec4 = vec4_ok and W % 4 == 0
    cpl = ((H * W + 15) // 16 + 63) // 64
    if vec4 and fast and (H, W) in ((16, 16), (32, 32), (64, 64)):
        return f"lds_{H}x{W}"                           # compile-time sizes
    if vec4 and fast:
        return "lds_rt_cpl1" if cpl == 1 else "lds_rt_vec4_fastdiv"  # runtime sizes, one chunk per lane / several
    if vec4:
        return "lds_rt_vec4_ieee"
    return "lds_rt_scalar_fastdiv" if fast else "lds_rt_scalar_ieee"


# one shape per forward route: 16x16 / 32x32 / 64x64 compile-time; 20x24 (480 cells: one chunk per lane), 40x60 (W 60: fast division,
# 3 chunks per lane), 30x36 (W 36: IEEE division) vec4; 20x45 (fast), 33x31 (IEEE) scalar; 96x96 (fast) and 80x80 (IEEE) from 6400 cells:
# the hybrid large-map kernel.  ("misaligned": 32x32 from a tensor 4 bytes off 16-byte alignment -> the scalar fast-division loop at W % 4 == 0)
ROUTE_SHAPES = {"lds_16x16": (16, 16), "lds_32x32": (32, 32), "lds_64x64": (64, 64), "lds_rt_cpl1": (20, 24), "lds_rt_vec4_fastdiv": (40, 60),
                "lds_rt_vec4_ieee": (30, 36), "lds_rt_scalar_fastdiv": (20, 45), "lds_rt_scalar_ieee": (33, 31), "hybrid_fastdiv": (96, 96),
                "hybrid_ieee": (80, 80)}
OTHER_SHAPES = [(12, 12), (24, 40), (48, 48), (7, 5), (9, 30), (36, 52), (70, 100), (64, 128), (90, 90), (100, 100), (1, 40), (40, 1), (5, 200)]


def misaligned(t):
    """the same values in a contiguous tensor 4 bytes off 16-byte alignment (the kernels' vec4 test fails: the scalar loop runs)"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    out = buf[1:].view(t.shape)
    out.copy_(t)
    return out


def masked_problems(rng, B, H, W, mask, p=0.15, max_dist=None, unsolvable_frac=0.0):
    """[B,1,H,W] maps / starts / goals: the goal reachable from the start under `mask` (tools/gen_golden_neighbors.reachable), or, with
    probability `unsolvable_frac` (and whenever nothing is reachable), a passable goal that is not -- or the start itself when there is none.
    max_dist: |dr|, |dc| <= max_dist (short searches on large maps)"""
    from gen_golden_neighbors import reachable
    filt = mask_filter(mask)
    maps = (rng.random((B, H, W)) > p).astype(np.float32)
    sidx, gidx = np.zeros(B, np.int64), np.zeros(B, np.int64)
    for b in range(B):
        s = int(rng.integers(H * W))
        maps[b].reshape(-1)[s] = 1.0
        r0 = c0 = 0
        win = maps[b]
        if max_dist is not None:  # (reachable inside a window around the start => reachable: the flood stays small on a large map)
            r0, c0 = max(0, s // W - 2 * max_dist), max(0, s % W - 2 * max_dist)
            win = maps[b, r0:s // W + 2 * max_dist + 1, c0:s % W + 2 * max_dist + 1]
        ws = (s // W - r0) * win.shape[1] + (s % W - c0)
        reach = reachable(win, ws, filt)
        reach[ws] = False
        wr, wc = np.divmod(np.flatnonzero(reach), win.shape[1])
        cand = (wr + r0) * W + (wc + c0)
        if max_dist is not None and cand.size:
            cand = cand[(np.abs(wr + r0 - s // W) <= max_dist) & (np.abs(wc + c0 - s % W) <= max_dist)]
        if cand.size == 0 or rng.random() < unsolvable_frac:
            if max_dist is None:
                cand = np.flatnonzero(~reach & (maps[b].reshape(-1) > 0))
            else:  # (outside the window: not necessarily unreachable -- the oracle decides either way)
                cand = np.flatnonzero(maps[b].reshape(-1) > 0)
            cand = cand[cand != s]
        sidx[b], gidx[b] = s, int(cand[rng.integers(cand.size)]) if cand.size else s
    onehot = np.zeros((2, B, H * W), np.float32)
    onehot[0, np.arange(B), sidx] = 1.0
    onehot[1, np.arange(B), gidx] = 1.0
    return maps[:, None], onehot[0].reshape(B, 1, H, W), onehot[1].reshape(B, 1, H, W)


def _draw_mask(rng):
    return int(rng.choice(NAMED_MASKS)) if rng.random() < 0.6 else int(rng.choice(MASKS_CENTRE_CLEAR))


def _draw_cost(rng, kind, maps, signed_ok=False):
    B, _, H, W = maps.shape
    if kind == "map":
        return maps
    if kind == "zeros":  # half the costs exactly zero: ties in g as well as in h
        return (rng.random((B, 1, H, W)) * (rng.random((B, 1, H, W)) < 0.5)).astype(np.float32)
    if kind == "signed":
        return rng.uniform(-0.5, 1.0, (B, 1, H, W)).astype(np.float32)
    if kind == "signed2":
        return rng.uniform(-2.0, 1.0, (B, 1, H, W)).astype(np.float32)
    return (rng.random((B, 1, H, W)) * (1.0 if kind == "u01" else 10.0)).astype(np.float32)


def compare_masked_search(out, o, want_log):
    """kernel outputs (hist, paths, iters, status, log) against the masked sm oracle: solved maps bit-exact incl. paths and logs; a map the
    neighbourhood cannot solve: the same status, closed set and step count (its path is undefined -- the reference raises there)"""
    hist, paths, iters, status, log = (None if x is None else x.cpu().numpy() for x in out)
    if not np.array_equal(status, o.map_status) or not np.array_equal(iters, o.iters) or not np.array_equal(hist, o.histories):
        return False
    for b in range(hist.shape[0]):
        if o.map_status[b] == 0 and not np.array_equal(paths[b], o.paths[b]):
            return False
        if want_log and not np.array_equal(log[b, :iters[b]], o.sel_log[b, :iters[b]]):
            return False
    return True


def run_masked(seed=7, N=120, verbose=True):
    """ops.search_nograd(..., neighbor_mask=m) -- nastar_forward_ex_masked, the masked twin of every compiled search kernel -- against the
    oracle's masked state machine: histories, paths, step counts, status codes and selection logs bit-exact.  Masks: single cells, Moore-8
    minus one cell, von Neumann, diagonals, uniform over all 256; start / goal placed by reachability under the mask (a tenth unsolvable);
    every route of `masked_route` (ROUTE_SHAPES first, then random shapes), misaligned views, random placements and logs where LDS-resident.
    -> (cases per route, failing case descriptions)"""
    rng = np.random.default_rng(seed)
    bad, stats = [], {}
    routes = list(ROUTE_SHAPES) + ["misaligned"]
    for case in range(N):
        if case < 2 * len(routes):
            r = routes[case % len(routes)]
            H, W = ROUTE_SHAPES.get(r, (32, 32))
        else:
            r = None
            H, W = OTHER_SHAPES[int(rng.integers(len(OTHER_SHAPES)))] if rng.random() < 0.4 else (int(rng.integers(2, 70)), int(rng.integers(2, 70)))
        mis = r == "misaligned" or (r is None and W % 4 == 0 and rng.random() < 0.15)
        large = not ops.in_lds(H, W)
        B = int(rng.integers(1, 3 if large else 7))
        mask = SINGLE_BIT_MASKS[case % 8] if case < 8 else _draw_mask(rng)
        maps, st, gl = masked_problems(rng, B, H, W, mask, p=float(rng.choice([0.0, 0.1, 0.25])), max_dist=12 if large else None,
                                       unsolvable_frac=0.1)
        kind = str(rng.choice(["map", "u01", "u10", "zeros"]))
        cost = _draw_cost(rng, kind, maps)
        gr = float(rng.choice([0.5, 0.5, 0.2, 0.8, 0.0, 1.0]))
        T = W * W if rng.random() < 0.8 else max(1, int(rng.choice([0.1, 0.5]) * W * W))
        log = bool(rng.random() < 0.5)
        order = None
        if not large and rng.random() < 0.4:
            order = torch.from_numpy(rng.permutation(B).astype(np.int32)).to(dev)
        c, s, g, m = (torch.from_numpy(np.ascontiguousarray(x[:, 0])).to(dev) for x in (cost, st, gl, maps))
        if mis:
            c = misaligned(c)
        route = masked_route(H, W, not mis)
        try:
            out = ops.search_nograd(c, s, g, c if kind == "map" else m, gr, T, want_log=log, order=order, check_order=False, neighbor_mask=mask)
            torch.cuda.synchronize()
            o = O.forward(cost, st, gl, maps, gr, T, mode="sm", want_log=log, neighbor_mask=mask)
            ok = compare_masked_search(out, o, log)
        except Exception as e:  # noqa: BLE001
            ok = False
            if verbose:
                print(json.dumps({"case": case, "error": f"{type(e).__name__}: {e}"[:300]}), flush=True)
        stats[route] = stats.get(route, 0) + 1
        if log and not large:
            stats["with_log"] = stats.get("with_log", 0) + 1
        if order is not None:
            stats["placed"] = stats.get("placed", 0) + 1
        if not ok:
            d = {"case": case, "H": H, "W": W, "B": B, "mask": hex(mask), "cost": kind, "g_ratio": gr, "max_iters": T, "log": log,
                 "placed": order is not None, "misaligned": mis, "route": route}
            bad.append(d)
            if verbose:
                print(json.dumps(d), flush=True)
    return stats, bad


def replay_route(H, W, max_iters):
    """the replay kernel nastar_backward_replay_ordered_masked launches (csrc/nastar_capi.hip backward_replay_impl): the compact state in LDS
    with or without the step history in LDS, or the state in the HBM workspace with 16- or 32-bit history stamps; fast / IEEE division"""
    HW = H * W
    HWp = (HW + 63) // 64 * 64
    hlen = min(max_iters, 2 * HW + 2) + 2
    wide = HW > 65535 - 16 or hlen > 65535
    lds = 160 * 1024
    st = HWp * 14 + 64
    div = "fastdiv" if W in FASTDIV_WIDTHS else "ieee"
    if not wide and st <= lds:
        with_hist = st + hlen * 16
        return ("replay_lds_hist_" if with_hist <= lds and (lds // with_hist >= 2 or lds // st < 2) else "replay_lds_state_") + div
    return ("replay_hbm32_" if wide else "replay_hbm16_") + div


# (H, W, training Tmax or None = eval): 32x32 and 33x31 eval keep the history in LDS (fast / IEEE); 64x64 and 60x66 eval do not (fast / IEEE);
# 120x120 and 112x128 keep the state in HBM (IEEE / fast; short training budgets: the dense oracle scans every cell per step)
BACKWARD_SHAPES = [(32, 32, None), (33, 31, None), (64, 64, None), (60, 66, None), (120, 120, 0.05), (112, 128, 0.05), (16, 16, 0.5),
                   (20, 45, 0.25), (12, 12, None), (24, 40, 0.5), (7, 5, None)]


def run_backward_masked(seed=13, N=22, verbose=True):
    """dL/dcost of DifferentiableAstar with a neighbor_filter under autograd (the masked replay backward) against the oracle's masked literal
    reverse mode, random upstream gradients; 1e-5 of scale.  -> (cases per replay route, failures)"""
    from neural_astar.planner.differentiable_astar import DifferentiableAstar
    rng = np.random.default_rng(seed)
    bad, stats = [], {}
    for case in range(N):
        H, W, Tmax = BACKWARD_SHAPES[case % len(BACKWARD_SHAPES)]
        train = Tmax is not None
        Tmax = Tmax if train else 1.0
        T = int(Tmax * W * W)
        big = H * W > 6000
        B = int(rng.integers(1, 3 if big else 5))
        mask = MOORE_MINUS_ONE_MASKS[case % 8] if case % 3 == 0 else _draw_mask(rng)
        maps, st, gl = masked_problems(rng, B, H, W, mask, p=float(rng.choice([0.0, 0.15])), max_dist=10 if big else None)
        cost_np = _draw_cost(rng, str(rng.choice(["u01", "u10", "zeros"])), maps)
        gr = float(rng.choice([0.5, 0.5, 0.2, 0.8]))
        o = O.forward(cost_np, st, gl, maps, gr, T, mode="dense", neighbor_mask=mask)
        if o.status:
            continue  # (a map the neighbourhood cannot solve within the budget has no gradient: the reference is NaN there)
        up = rng.standard_normal((B, 1, H, W)).astype(np.float32)
        da = DifferentiableAstar(gr, Tmax).to(dev).train(train)
        with torch.no_grad():
            da.neighbor_filter.copy_(torch.tensor(mask_filter(mask), dtype=torch.float32).reshape(1, 1, 3, 3))
        cost = torch.from_numpy(cost_np).to(dev).requires_grad_(True)
        s, g, m = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (st, gl, maps))
        route = replay_route(H, W, T)
        try:
            out = da(cost, s, g, m)
            (out.histories * torch.from_numpy(up).to(dev)).sum().backward()
            ref = O.backward(up, cost_np, st, gl, maps, gr, T, neighbor_mask=mask)
            err = float(np.abs(cost.grad[:, 0].cpu().numpy() - ref).max())
            ok = err <= 1e-5 * max(1.0, float(np.abs(ref).max())) and np.array_equal(out.histories[:, 0].detach().cpu().numpy(), o.histories)
        except Exception as e:  # noqa: BLE001
            ok, err = False, f"{type(e).__name__}: {e}"[:300]
        stats[route] = stats.get(route, 0) + 1
        if not ok:
            d = {"case": case, "H": H, "W": W, "B": B, "mask": hex(mask), "g_ratio": gr, "train": train, "Tmax": Tmax, "route": route, "err": err}
            bad.append(d)
            if verbose:
                print(json.dumps(d), flush=True)
    return stats, bad


def run_module_masked(seed=17, N=60, verbose=True, grad_frac=0.3, large_every=10, large_hw=(96, 96)):
    """DifferentiableAstar.forward() with a neighbor_filter against the oracle's masked LITERAL batch loop: g_ratio 0 / 0.2 / 0.5 / 0.8 / 1,
    costs up to 10, signed, half exactly zero; every checking mode; a share under autograd.  Batches in the coupled class (a finished map not
    at a fixed point of the batch loop: the masked dense and sm restatements differ) go through the lock-step re-run of
    nastar_forward_batchloop_finish_masked; every `large_every`-th case is on a hybrid-sized map (the masked lock-step large-map kernel).
    -> (cases, coupled batches, coupled batches on hybrid-sized maps, gradient cases, failures)"""
    import warnings
    from neural_astar.planner.differentiable_astar import DifferentiableAstar
    rng = np.random.default_rng(seed)
    bad, n, reruns, reruns_large, ngrad = [], 0, 0, 0, 0
    for case in range(N):
        large = case % large_every == large_every - 1
        if large:
            H, W = large_hw
        else:
            H, W = (int(rng.integers(4, 36)), int(rng.integers(4, 36))) if rng.random() < 0.8 else (int(rng.choice([16, 32])),) * 2
        B = int(rng.integers(2, 4 if large else 6))
        mask = _draw_mask(rng)
        maps, st, gl = masked_problems(rng, B, H, W, mask, p=float(rng.choice([0.0, 0.1, 0.25])), max_dist=6 if large else None)
        kind = str(rng.choice(["map", "u01", "u10", "u10", "zeros", "signed", "signed2"]))
        if large:
            kind = str(rng.choice(["u01", "zeros"]))
        cost = _draw_cost(rng, kind, maps)
        gr = float(rng.choice([0.0, 0.2, 0.2, 0.5, 0.8, 1.0])) if not large else float(rng.choice([0.0, 0.2]))
        if large:  # an expensive goal cell at g_ratio < 0.5: its expansion opens cells that beat it (the coupled class)
            cost = cost.copy()
            cost.reshape(B, -1)[np.arange(B), gl.reshape(B, -1).argmax(1)] = 10.0
        train = bool(rng.random() < 0.3) and not large
        Tmax = float(rng.choice([0.25, 0.5])) if train else 1.0
        T = int(Tmax * W * W) if train else W * W
        if T < 1:
            continue
        o = O.forward(cost, st, gl, maps, gr, T, mode="dense", neighbor_mask=mask)
        if o.status:
            continue  # (an empty open list: the reference crashes there)
        osm = O.forward(cost, st, gl, maps, gr, T, mode="sm", neighbor_mask=mask)
        coupled = not np.array_equal(o.histories, osm.histories)
        reruns += int(coupled)
        reruns_large += int(coupled and large)
        with_grad = kind != "map" and rng.random() < grad_frac and not large
        mode = [True, "deferred", False][int(rng.integers(0, 3))]
        if mode is False and not ops.coupling_possible(gr):
            mode = True  # (unchecked calls read nothing back: only costs below -1 reach the class at this g_ratio)
        if mode == "deferred" and with_grad and not ops.coupling_possible(gr):
            mode = True  # (deferred + autograd + costs below -1: refused by design)
        da = DifferentiableAstar(gr, Tmax, check_solvable=mode).to(dev).train(train)
        with torch.no_grad():
            da.neighbor_filter.copy_(torch.tensor(mask_filter(mask), dtype=torch.float32).reshape(1, 1, 3, 3))
        c, s, g, m = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (cost, st, gl, maps))
        err = None
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("error")
                if with_grad:
                    up = rng.standard_normal((B, 1, H, W)).astype(np.float32)
                    cg = c.clone().requires_grad_(True)
                    out = da(cg, s, g, m)
                    (out.histories * torch.from_numpy(up).to(dev)).sum().backward()
                    da.raise_if_unsolvable()
                    ref = O.backward(up, cost, st, gl, maps, gr, T, neighbor_mask=mask)
                    gerr = float(np.abs(cg.grad[:, 0].cpu().numpy() - ref).max())
                    ngrad += 1
                    if not gerr <= 1e-5 * max(1.0, float(np.abs(ref).max())):
                        err = f"grad err {gerr:.3e} (scale {float(np.abs(ref).max()):.3e})"
                else:
                    with torch.no_grad():
                        out = da(c, s, g, c if kind == "map" else m)
                        da.raise_if_unsolvable()
            if not (np.array_equal(out.histories[:, 0].detach().cpu().numpy(), o.histories) and np.array_equal(out.paths[:, 0].cpu().numpy(), o.paths)):
                err = "histories / paths differ from the literal batch loop"
        except Exception as e:  # noqa: BLE001
            err = f"{type(e).__name__}: {e}"[:300]
        n += 1
        if err:
            d = {"case": case, "H": H, "W": W, "B": B, "mask": hex(mask), "cost": kind, "g_ratio": gr, "train": train, "mode": str(mode),
                 "grad": bool(with_grad), "coupled": coupled, "error": err}
            bad.append(d)
            if verbose:
                print(json.dumps(d), flush=True)
    run_module_masked.ngrad = ngrad
    return n, reruns, reruns_large, bad


if __name__ == "__main__" and len(sys.argv) > 1 and sys.argv[1] == "masked":
    # python tools/fuzz_parity.py masked <seed> <N>: the masked kernels only (search sweep N cases, backward N/5, module N/2)
    seed_m = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    n_m = int(sys.argv[3]) if len(sys.argv) > 3 else 400
    st_m, bad_s = run_masked(seed=seed_m, N=n_m)
    print(json.dumps({"masked_cases": sum(v for k, v in st_m.items() if k not in ("with_log", "placed")), "by_route": st_m, "mismatches": len(bad_s)}))
    st_b, bad_bm = run_backward_masked(seed=seed_m + 1, N=max(11, n_m // 5))
    print(json.dumps({"masked_backward_by_route": st_b, "failures": len(bad_bm)}))
    nm, rr, rrl, bad_mm = run_module_masked(seed=seed_m + 2, N=max(20, n_m // 2))
    print(json.dumps({"masked_module_cases": nm, "coupled": rr, "coupled_hybrid": rrl, "gradient_cases": run_module_masked.ngrad,
                      "failures": len(bad_mm)}))
    sys.exit(1 if (bad_s or bad_bm or bad_mm) else 0)


if __name__ == "__main__" and len(sys.argv) > 1 and sys.argv[1] == "module":
    # python tools/fuzz_parity.py module <seed> <N>: only the module sweep (every mode, autograd, large maps) against the literal batch loop
    # (a 4th argument "small": large maps only to 125x130 -- the oracle's dense restatement needs tens of seconds for one 150x200 batch)
    small = len(sys.argv) > 4 and sys.argv[4] == "small"
    nm, rr, bad_m = run_module(seed=int(sys.argv[2]) if len(sys.argv) > 2 else 31, N=int(sys.argv[3]) if len(sys.argv) > 3 else 300,
                               **({"large_frac": 0.06, "large_hw": ((112, 126), (112, 131))} if small else {}))
    print(json.dumps({"module_vs_literal_batch_loop_cases": nm, "batches_in_the_coupled_class": rr, "gradient_cases": run_module.ngrad, "module_failures": len(bad_m)}))
    sys.exit(1 if bad_m else 0)

if __name__ == "__main__":
    st, bad_cases = run(int(sys.argv[1]) if len(sys.argv) > 1 else 20260926, int(sys.argv[2]) if len(sys.argv) > 2 else 160,
                        float(sys.argv[3]) if len(sys.argv) > 3 else 0.15)
    print(json.dumps({"cases": sum(st.values()), "by_kernel": st, "mismatches": len(bad_cases)}))
    nb, bad_b = run_backward(N=max(20, (int(sys.argv[2]) if len(sys.argv) > 2 else 160) // 10))
    print(json.dumps({"backward_cases": nb, "backward_failures": len(bad_b)}))
    bad_l = []
    if len(sys.argv) > 4:  # a few LARGE backward cases (seconds of oracle time each)
        nl, bad_l = run_backward(seed=5, N=int(sys.argv[4]), large=True)
        print(json.dumps({"backward_large_cases": nl, "backward_large_failures": len(bad_l)}))
    nm, rr, bad_m = run_module(N=int(sys.argv[6]) if len(sys.argv) > 6 else 60)
    print(json.dumps({"module_vs_literal_batch_loop_cases": nm, "batches_in_the_coupled_class": rr, "gradient_cases": run_module.ngrad, "module_failures": len(bad_m)}))
    if bad_m:
        sys.exit(1)
    ne, bad_e = run_encoder(N=int(sys.argv[5]) if len(sys.argv) > 5 else 40)
    print(json.dumps({"encoder_cases": ne, "encoder_failures": len(bad_e), "routes": run_encoder.routes}))
    sys.exit(1 if (bad_cases or bad_b or bad_l or bad_e) else 0)
