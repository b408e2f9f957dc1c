"""ctypes binding of the C ABI in ``include/nastar.h`` (``lib/libnastar_hip.so``).

This is the ONLY compute path of the package: there is no CPU or PyTorch fallback.  If the shared library is
missing the import of the planner still succeeds (so that CPU-only tooling can inspect the modules) but the
first call fails loudly with instructions to build it.
"""
from __future__ import annotations

import ctypes
import os
import subprocess
from typing import Optional

_PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))  # neural-astar_amd/
# NASTAR_LIB: development switch -- another build of the same C ABI (make BUILD=build_x OUT=../lib/libnastar_hip_x.so)
LIB_PATH = os.environ.get("NASTAR_LIB") or os.path.join(_PKG_ROOT, "lib", "libnastar_hip.so")
CSRC_DIR = os.path.join(_PKG_ROOT, "csrc")

NASTAR_OK = 0
NASTAR_ERR_BAD_SHAPE = 1
NASTAR_ERR_UNSUPPORTED = 2
NASTAR_ERR_UNSOLVABLE = 3
NASTAR_ERR_HIP = 4
NASTAR_ERR_NULL = 5
NASTAR_ERR_WORKSPACE = 6
NASTAR_ERR_NOT_UNIT_COST = 7  # per-map status only
NASTAR_ERR_BAD_HEURISTIC = 8  # per-map status only
NASTAR_ERR_BAD_COST = 9  # per-map status of include/nastar_fields.h only
NASTAR_ERR_NO_CONVERGENCE = 10  # per-map status of include/nastar_fields.h only
NASTAR_ERR_PLATEAU = 11  # per-map status of include/nastar_fields_grad.h only

_ERR_NAMES = {
    NASTAR_ERR_BAD_SHAPE: "bad shape (B, H, W and max_iters must be positive)",
    NASTAR_ERR_UNSUPPORTED: "map size not supported by the implemented kernels",
    NASTAR_ERR_UNSOLVABLE: "unsolvable map",
    NASTAR_ERR_HIP: "HIP runtime error",
    NASTAR_ERR_NULL: "NULL pointer argument",
    NASTAR_ERR_WORKSPACE: "workspace too small",
    NASTAR_ERR_NOT_UNIT_COST: "NASTAR_FLAG_UNIT_COST was passed for a map that holds a value other than 0.0 / 1.0",
    NASTAR_ERR_BAD_HEURISTIC: "a NaN or an infinite value in a map's heuristic",
}

# ---- the signatures of include/nastar.h, each written ONCE: "<return type> <argument types>", one letter per C type (tests/test_capi_library.py
# compares every entry with the header's prototype).  load() / load_dev() turn them into ctypes restype / argtypes.
_CTYPES = {"p": ctypes.c_void_p,                  # any pointer (device or host); NULL = None
           "P": ctypes.POINTER(ctypes.c_void_p),  # pointer to pointer: a HOST array of device pointers
           "i": ctypes.c_int, "u": ctypes.c_uint, "f": ctypes.c_float, "d": ctypes.c_double, "z": ctypes.c_size_t, "q": ctypes.c_longlong,
           "s": ctypes.c_char_p}                  # (return type only: const char*)
_MAPS = "pppp"            # cost, start, goal, passable
_BUDGET = "iiidi"         # B, H, W, g_ratio, max_iters
_OUTPUTS = "ppppp"        # histories_out, paths_out, sel_log_out, iters_out, status_out
_WORKSPACE = "pz"         # workspace, workspace_bytes
_FORWARD = _MAPS + _BUDGET + _OUTPUTS
_REPLAY = _MAPS + "p" + _BUDGET + "ppp" + _WORKSPACE  # ..., sel_log, ..., iters, t_batch_dev, grad_cost_out, ...


def _family(name: str, args: str) -> dict:
    """an entry point whose last argument is the stream, and its twins `_masked` (`unsigned neighbor_mask` in front of the stream) and
    `_heuristic` (`unsigned neighbor_mask, const float* h0`)"""
    return {name: "i " + args + "p", name + "_masked": "i " + args + "up", name + "_heuristic": "i " + args + "upp"}


SIGNATURES = {
    "nastar_version": "i ",
    "nastar_last_error": "s ",
    "nastar_workspace_bytes": "z iiii",
    "nastar_forward": "i " + _FORWARD + _WORKSPACE + "ip",
    "nastar_forward_packed": "i " + _FORWARD + "p" + _WORKSPACE + "ip",
    "nastar_forward_ordered": "i " + _FORWARD + "p" + _WORKSPACE + "ippp",
    # ... packed_out, workspace, workspace_bytes, flags, order, order_out, status_summary, completion_counter
    **_family("nastar_forward_ex", _FORWARD + "p" + _WORKSPACE + "ipppp"),
    "nastar_batchloop_workspace_bytes": "z iiii",
    **_family("nastar_forward_batchloop_finish", _FORWARD + _WORKSPACE),
    "nastar_completion_supported": "i ii",
    "nastar_host_wait_nonzero": "i pi",
    "nastar_placement_from_levels": "i pipp",
    "nastar_placement_predict": "i pppiiippzp",
    "nastar_backward_workspace_bytes": "z iiii",
    "nastar_backward_replay": "i p" + _REPLAY + "ip",
    # grad_histories, histories, opt_trajs, grad_loss_dev, ..., flags, order
    **_family("nastar_backward_replay_ordered", "pppp" + _REPLAY + "ip"),
    "nastar_backward_l1_replay": "i ppp" + _REPLAY + "p",
    "nastar_l1_loss": "i ppqppzp",
    "nastar_policy_rollout": "i pppiiiiippp",
    "nastar_heuristic": "i piiipp",
    "nastar_debug_occupancy": "i iip",
    "nastar_pack_outputs": "i ppiiipp",
    "nastar_unpack_outputs": "i piiippp",
    "nastar_encoder_workspace_bytes": "z iii",
    "nastar_encoder_cnn_forward": "i pppiiiiPPPfppzp",
    "nastar_encoder_workspace_bytes_f16x3": "z iii",
    "nastar_encoder_cnn_forward_f16x3": "i pppiiiipPPPfppzp",
    "nastar_encoder_workspace_bytes_f16": "z iii",
    "nastar_encoder_cnn_forward_f16": "i pppiiiipPPPfppzp",
    "nastar_conv3x3_bf16": "i pppppiiiiiip",
    "nastar_encoder_downsize_workspace_bytes": "z iiiii",
    "nastar_encoder_cnn_downsize_forward": "i pppiiiiiiiiPPPfppzp",
    "nastar_conv3x3_f16": "i pppppppiiiiiiifp",
    "nastar_conv3x3_img32_f16": "i pppppiiiip",
    "nastar_maxpool2x2_f16": "i ppiiiiip",
    "nastar_encoder_prep_f16": "i pppiqiipp",
    "nastar_conv3x3_wgrad_workspace_bytes": "z iiiii",
    "nastar_conv3x3_wgrad_f16": "i pppiiiiiiiifppzp",
    "nastar_chan_stats_f16": "i ppppppqiip",
    "nastar_chan_stats_workspace_bytes": "z qi",
    "nastar_absmax_multi_f32": "i pipp",
    "nastar_pack_conv_weights_multi_f16": "i piiipppp",
    "nastar_rmsprop_multi_f32": "i pifffp",
    "nastar_bn1_parts": "i q",
    "nastar_bn1_fwd_partial": "i pqpp",
    "nastar_bn1_sigmoid_fwd": "i pqpidppdpdppppp",
    "nastar_bn1_sigmoid_bwd_partial": "i ppqpppppp",
    "nastar_bn1_sigmoid_bwd": "i ppqpppppidppppp",
    "nastar_chan_stats_f16_ws": "i ppppppqiipzp",
    "nastar_chan_affine_f16": "i ppppppppqiiip",
    "nastar_pack_conv_weight_f16": "i piiiipppppip",
    "nastar_bn_coef_fwd": "i pppdqdppppppip",
    "nastar_bn_coef_bwd": "i pppppqppppppip",
    "nastar_bn_coef_bwd_io": "i pppppqpppppppip",
    "nastar_bn_stats_coef_fwd_f16": "i pqiippddppppppppzp",
    "nastar_bn_stats_coef_bwd_f16": "i ppppqiippppppppppppzp",
    "nastar_grad_seed_f16": "i pqipppp",
    "nastar_conv3x3_co1_workspace_bytes": "z iiii",
    "nastar_conv3x3_co1_f16": "i pppiiiiippppzp",
    "nastar_conv3x3_co1_wgrad_f16": "i ppiiiiippppzp",
    "nastar_grad_scale_f32": "i pqppp",
    "nastar_bn_stats_coef_bwd_u1_f16": "i ppiiipppiippppppppppppzp",
    "nastar_chan_affine_u1_f16": "i pppiiipppppppiip",
    "nastar_chan_stats_u1_f16_ws": "i pppiiipppppiipzp",
    "nastar_maxpool2x2_bwd_f16": "i pppiiiiip",
    "nastar_upcat_f16": "i pppiiiiiip",
    "nastar_upcat_bwd_f16": "i pppiiiiiip",
    "nastar_grad_add_f16": "i ppppppqiip",
}

# every symbol include/nastar.h declares -- tests check the library exports all of them
EXPORTED_SYMBOLS = tuple(SIGNATURES)

# the signatures of include/nastar_routes.h (the second header: ordered routes, lengths and costs from the search launch), same letter code;
# a table of its own -- SIGNATURES is include/nastar.h and nothing else (tests/test_routes.py compares this one with ITS header)
_ROUTES = "pipp"          # routes_out, route_cap, route_len_out, route_cost_out
ROUTE_SIGNATURES = {
    "nastar_routes_abi": "i ",
    # ... nastar_forward_ex_heuristic's arguments (h0 may be NULL), the route outputs, the stream
    "nastar_forward_routes": "i " + _FORWARD + "p" + _WORKSPACE + "ipppp" + "up" + _ROUTES + "p",
    "nastar_forward_routes_batchloop_finish": "i " + _FORWARD + _WORKSPACE + "up" + _ROUTES + "p",
}

# the signatures of include/nastar_sources.h (the third header: the search from every non-zero cell of the start map, and its replay), same
# letter code; again a table of its own (tests/test_multisource.py compares it with ITS header)
SOURCE_SIGNATURES = {
    "nastar_sources_abi": "i ",
    # ... the arguments of nastar_forward_routes (h0 and the route outputs may be NULL)
    "nastar_forward_sources": "i " + _FORWARD + "p" + _WORKSPACE + "ipppp" + "up" + _ROUTES + "p",
    "nastar_forward_sources_batchloop_finish": "i " + _FORWARD + _WORKSPACE + "up" + _ROUTES + "p",
    # ... the arguments of nastar_backward_replay_ordered_heuristic (h0 may be NULL)
    "nastar_backward_replay_sources": "i pppp" + _REPLAY + "ip" + "upp",
}

# the signatures of include/nastar_levels.h (the fourth header: the search launch that places its maps by their levels itself), same letter
# code; a table of its own (tests/test_levels_in_launch.py compares it with ITS header)
LEVEL_SIGNATURES = {
    "nastar_levels_abi": "i ",
    # ... nastar_forward_ex's arguments with `levels` in place of order, order_out
    "nastar_forward_levels": "i " + _FORWARD + "p" + _WORKSPACE + "ippp" + "p",
    "nastar_levels_in_launch": "i iiii",
    "nastar_placement_slots": "i pipp",
}

# the signatures of include/nastar_fields.h (the fifth header: the cost-to-go field of whole maps and its optimal policy), same letter code;
# a table of its own (tests/test_fields.py compares it with ITS header)
FIELD_SIGNATURES = {
    "nastar_fields_abi": "i ",
    "nastar_fields_max_cells": "i ",
    # cost, goal, passable, B, H, W, neighbor_mask, dist_out, policy_out, status_out, (sweeps_out,) stream
    "nastar_cost_to_go": "i pppiiiupppp",
    "nastar_cost_to_go_sweeps": "i pppiiiuppppp",
}

# the signatures of include/nastar_fields_tiled.h (the sixth header: the same field for maps of up to 1179648 cells, by a tiled relaxation),
# same letter code; a table of its own (tests/test_fields_tiled.py compares it with ITS header)
TILED_FIELD_SIGNATURES = {
    "nastar_fields_tiled_abi": "i ",
    "nastar_fields_tiled_max_cells": "i ",
    "nastar_fields_tile": "i pp",
    "nastar_cost_to_go_tiled_workspace_bytes": "z iii",
    # cost, goal, passable, B, H, W, neighbor_mask, dist_out, policy_out, status_out, visits_out, workspace, workspace_bytes, max_rounds,
    # (launches_per_batch,) rounds_out, stream
    "nastar_cost_to_go_tiled": "i pppiiiupppppzqpp",
    "nastar_cost_to_go_tiled_batched": "i pppiiiupppppzqipp",
}

# the signatures of include/nastar_verdict.h (the seventh header: the proof, launched beside a search, that every map of the batch is
# solvable), same letter code; a table of its own (tests/test_verdict_proof.py compares it with ITS header)
VERDICT_SIGNATURES = {
    "nastar_verdict_abi": "i ",
    "nastar_solvable_proof_supported": "i ii",
    # cost, start, goal, passable, B, H, W, proved_out, word, counter, stream
    "nastar_solvable_proof": "i " + _MAPS + "iii" + "pppp",
    "nastar_solvable_proof_sync": "i ",
}

# the signatures of include/nastar_ticket.h (the sixteenth header: a search launch and the proof of its batch from one call, the proof ordered
# behind the search launch's own start), same letter code; a table of its own (tests/test_proof_ticket.py compares it with ITS header)
TICKET_SIGNATURES = {
    "nastar_ticket_abi": "i ",
    "nastar_proof_ticket_available": "i ",
    "nastar_proof_order_counts": "i pp",
    # the arguments of nastar_forward_ex up to completion_counter, levels, proved_out, proof_word, proof_counter, proof_rc, stream
    "nastar_forward_proved": "i " + _FORWARD + "p" + _WORKSPACE + "ipppp" + "ppppp" + "p",
}

# the signatures of include/nastar_fields_grad.h (the eighth header: the gradient of the cost-to-go field with respect to the cost maps), same
# letter code; a table of its own (tests/test_fields_grad.py compares it with ITS header)
FIELD_GRAD_SIGNATURES = {
    "nastar_fields_grad_abi": "i ",
    "nastar_fields_grad_max_cells": "i ",
    # dist, goal, passable, grad_dist, B, H, W, neighbor_mask, grad_cost_out, status_out, sweeps_out, stream
    "nastar_fields_backward": "i ppppiiiupppp",
}

# the signatures of include/nastar_fields_grad_tiled.h (the ninth header: that gradient for maps of up to 1179648 cells, by a tiled subtree
# sum), same letter code; a table of its own (tests/test_fields_grad_tiled.py compares it with ITS header)
FIELD_GRAD_TILED_SIGNATURES = {
    "nastar_fields_grad_tiled_abi": "i ",
    "nastar_fields_grad_tiled_max_cells": "i ",
    "nastar_fields_backward_tiled_workspace_bytes": "z iii",
    # dist, goal, passable, grad_dist, B, H, W, neighbor_mask, grad_cost_out, status_out, visits_out, workspace, workspace_bytes, max_rounds,
    # rounds_out, stream
    "nastar_fields_backward_tiled": "i ppppiiiuppppzqpp",
    # dist, goal, passable, B, H, W, neighbor_mask, status_out, workspace, workspace_bytes, stream
    "nastar_fields_backward_tiled_status": "i pppiiiuppzp",
}

# the signatures of include/nastar_field_routes.h (the tenth header: ordered optimal routes for many start cells per map, read off a
# cost-to-go field), same letter code; a table of its own (tests/test_field_routes.py compares it with ITS header)
FIELD_ROUTE_SIGNATURES = {
    "nastar_field_routes_abi": "i ",
    "nastar_field_routes_max_cells": "i ",
    "nastar_field_routes_lds_cells": "i ",
    "nastar_field_routes_workspace_bytes": "z iii",
    # dist, goal, passable, start_idx, B, S, H, W, neighbor_mask, routes_out, route_cap, route_len_out, route_cost_out, status_out, workspace,
    # workspace_bytes, stream
    "nastar_field_routes": "i ppppiiiiupippppzp",
}

# the signatures of include/nastar_path_masks.h (the eleventh header: the exact shortest path of every map as a 0/1 mask, and its blackbox
# gradient with respect to the costs), same letter code; a table of its own (tests/test_path_masks.py compares it with ITS header)
PATH_MASK_SIGNATURES = {
    "nastar_path_masks_abi": "i ",
    "nastar_path_masks_max_cells": "i ",
    # cost, goal, passable, start_idx, B, H, W, neighbor_mask, path_out, path_cost_out, status_out, stream
    "nastar_path_masks": "i ppppiiiupppp",
    # cost, goal, passable, start_idx, grad_path, path_fwd, status_fwd, B, H, W, neighbor_mask, lambda, min_cost, grad_cost_out, status_out, stream
    "nastar_path_masks_backward": "i pppppppiiiuffppp",
}

# the signatures of include/nastar_path_masks_tiled.h (the twelfth header: that mask and that gradient for maps of up to 1179648 cells, the
# field by the tiled relaxation), same letter code; a table of its own (tests/test_path_masks_tiled.py compares it with ITS header)
PATH_MASK_TILED_SIGNATURES = {
    "nastar_path_masks_tiled_abi": "i ",
    "nastar_path_masks_tiled_max_cells": "i ",
    "nastar_path_masks_tiled_workspace_bytes": "z iii",
    "nastar_path_masks_tiled_backward_workspace_bytes": "z iii",
    # cost, goal, passable, start_idx, B, H, W, neighbor_mask, path_out, path_cost_out, status_out, workspace, workspace_bytes, max_rounds,
    # rounds_out, stream
    "nastar_path_masks_tiled": "i ppppiiiuppppzqpp",
    # cost, goal, passable, start_idx, grad_path, path_fwd, status_fwd, B, H, W, neighbor_mask, lambda, min_cost, grad_cost_out, status_out,
    # workspace, workspace_bytes, max_rounds, rounds_out, stream
    "nastar_path_masks_tiled_backward": "i pppppppiiiuffpppzqpp",
}

# the signatures of include/nastar_soft_fields.h (the thirteenth header: the entropy-regularised cost-to-go field over a finite horizon, its
# soft policy and its gradient with respect to the costs), same letter code; a table of its own (tests/test_soft_fields.py compares it with
# ITS header)
SOFT_FIELD_SIGNATURES = {
    "nastar_soft_fields_abi": "i ",
    "nastar_soft_fields_max_cells": "i ",
    "nastar_soft_fields_grad_max_cells": "i ",
    "nastar_soft_fields_tape_bytes": "z iiii",
    # cost, goal, passable, B, H, W, neighbor_mask, tau, horizon, dist_out, policy_out, status_out, tape, tape_bytes, stream
    "nastar_soft_cost_to_go": "i pppiiiudippppzp",
    # cost, goal, passable, tape, tape_bytes, grad_dist, B, H, W, neighbor_mask, tau, horizon, grad_cost_out, status_out, stream
    "nastar_soft_fields_backward": "i ppppzpiiiudippp",
}

# the signatures of include/nastar_soft_fields_tiled.h (the fourteenth header: the same field and gradient by tiled sweeps, with a checkpointed
# tape, for maps of up to 1024 x 1152), same letter code; a table of its own (tests/test_soft_fields_tiled.py compares it with ITS header)
SOFT_FIELD_TILED_SIGNATURES = {
    "nastar_soft_fields_tiled_abi": "i ",
    "nastar_soft_fields_tiled_max_cells": "i ",
    "nastar_soft_fields_tile": "i ppp",                                # th, tw, sweeps: host ints
    "nastar_soft_fields_tiled_workspace_bytes": "z iii",
    "nastar_soft_fields_tiled_tape_bytes": "z iiiii",                  # B, H, W, horizon, checkpoint_every
    "nastar_soft_fields_tiled_backward_workspace_bytes": "z iiiii",
    # cost, goal, passable, B, H, W, neighbor_mask, tau, horizon, dist_out, policy_out, status_out, tape, tape_bytes, checkpoint_every, workspace,
    # workspace_bytes, stream
    "nastar_soft_cost_to_go_tiled": "i pppiiiudippppzipzp",
    # ... workspace_bytes, sweeps_per_launch, stream
    "nastar_soft_cost_to_go_tiled_with_sweeps": "i pppiiiudippppzipzip",
    # cost, goal, passable, tape, tape_bytes, checkpoint_every, grad_dist, B, H, W, neighbor_mask, tau, horizon, grad_cost_out, status_out,
    # workspace, workspace_bytes, stream
    "nastar_soft_fields_backward_tiled": "i ppppzipiiiudipppzp",
}

# the signatures of include/nastar_soft_policy.h (the fifteenth header: the log-policy of the thirteenth's field and the gradient through
# it), same letter code; a table of its own (tests/test_soft_policy.py compares it with ITS header)
SOFT_POLICY_SIGNATURES = {
    "nastar_soft_policy_abi": "i ",
    # cost, goal, passable, B, H, W, neighbor_mask, tau, horizon, dist_out, policy_out, log_policy_out, status_out, tape, tape_bytes, stream
    "nastar_soft_policy_forward": "i pppiiiudipppppzp",
    # cost, goal, passable, tape, tape_bytes, grad_dist, grad_log_policy, B, H, W, neighbor_mask, tau, horizon, grad_cost_out, status_out, stream
    "nastar_soft_policy_backward": "i ppppzppiiiudippp",
}

# the signatures of include/nastar_soft_policy_tiled.h (the seventeenth header: the fifteenth's log-policy and gradient by the fourteenth's
# tiled sweeps and checkpointed tape), same letter code; a table of its own (tests/test_soft_policy_tiled.py compares it with ITS header)
SOFT_POLICY_TILED_SIGNATURES = {
    "nastar_soft_policy_tiled_abi": "i ",
    "nastar_soft_policy_tiled_backward_workspace_bytes": "z iiiii",   # B, H, W, horizon, checkpoint_every
    # cost, goal, passable, B, H, W, neighbor_mask, tau, horizon, dist_out, policy_out, log_policy_out, status_out, tape, tape_bytes,
    # checkpoint_every, workspace, workspace_bytes, stream
    "nastar_soft_policy_forward_tiled": "i pppiiiudipppppzipzp",
    # ... workspace_bytes, sweeps_per_launch, stream
    "nastar_soft_policy_forward_tiled_with_sweeps": "i pppiiiudipppppzipzip",
    # cost, goal, passable, tape, tape_bytes, checkpoint_every, grad_dist, grad_log_policy, B, H, W, neighbor_mask, tau, horizon,
    # grad_cost_out, status_out, workspace, workspace_bytes, stream
    "nastar_soft_policy_backward_tiled": "i ppppzippiiiudipppzp",
}

# the signatures of include/nastar_soft_routes.h (the eighteenth header: sampled routes from the maximum-entropy route distribution of the
# thirteenth's field), same letter code; a table of its own (tests/test_soft_routes.py compares it with ITS header)
SOFT_ROUTE_SIGNATURES = {
    "nastar_soft_routes_abi": "i ",
    "nastar_soft_routes_max_cells": "i ",
    # cost, goal, passable, tape, tape_bytes, start_idx, B, S, N, H, W, neighbor_mask, tau, horizon, seed, uniforms, routes_out, route_cap,
    # route_len_out, route_cost_out, log_prob_out, visits_out, status_out, stream
    "nastar_soft_routes": "i ppppzpiiiiiudiqppipppppp",
    # ... status_out, shape, stream
    "nastar_soft_routes_with_shape": "i ppppzpiiiiiudiqppipppppip",
}

# the signatures of include/nastar_soft_routes_tiled.h (the nineteenth header: the eighteenth's samples from the fourteenth's checkpointed
# tape), same letter code; a table of its own (tests/test_soft_routes_tiled.py compares it with ITS header)
SOFT_ROUTES_TILED_SIGNATURES = {
    "nastar_soft_routes_tiled_abi": "i ",
    "nastar_soft_routes_tiled_max_cells": "i ",
    "nastar_soft_routes_tiled_workspace_bytes": "z iiiiiii",          # B, S, N, H, W, horizon, checkpoint_every
    # cost, goal, passable, tape, tape_bytes, checkpoint_every, start_idx, B, S, N, H, W, neighbor_mask, tau, horizon, seed, uniforms,
    # routes_out, route_cap, route_len_out, route_cost_out, log_prob_out, visits_out, status_out, workspace, workspace_bytes, stream
    "nastar_soft_routes_tiled": "i ppppzipiiiiiudiqppippppppzp",
}

# the signatures of include/nastar_soft_routes_grad.h (the twentieth header: the score-function backward of the eighteenth's samples), same
# letter code; a table of its own (tests/test_soft_routes_grad.py compares it with ITS header)
SOFT_ROUTES_GRAD_SIGNATURES = {
    "nastar_soft_routes_grad_abi": "i ",
    "nastar_soft_routes_grad_max_cells": "i ",
    "nastar_soft_routes_grad_workspace_bytes": "z iii",
    # cost, goal, passable, tape, tape_bytes, start_idx, routes, route_cap, route_len, status, grad_log_prob, B, S, N, H, W, neighbor_mask,
    # tau, horizon, grad_cost_out, status_out, workspace, workspace_bytes, stream
    "nastar_soft_routes_backward": "i ppppzppipppiiiiiudipppzp",
}


class NativeLibraryMissing(RuntimeError):
    pass


_lib: Optional[ctypes.CDLL] = None


def build(verbose: bool = False) -> str:
    """Compile the HIP extension in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    out = None if verbose else subprocess.DEVNULL
    subprocess.check_call(["make", "-C", CSRC_DIR], stdout=out)
    return LIB_PATH


DEV_LIB_PATH = os.path.join(_PKG_ROOT, "lib", "libnastar_hip_dev.so")
_dev_lib: Optional[ctypes.CDLL] = None


def _bind(lib: ctypes.CDLL, names, table=None) -> None:
    table = SIGNATURES if table is None else table
    for name in names:
        ret, args = table[name].split(" ")
        fn = getattr(lib, name)
        fn.restype = _CTYPES[ret]
        fn.argtypes = [_CTYPES[k] for k in args]


def _bind_search(lib: ctypes.CDLL) -> None:
    """the search entry points the development build is called through (the product library binds every symbol)"""
    _bind(lib, ("nastar_workspace_bytes", "nastar_forward_ex", "nastar_batchloop_workspace_bytes", "nastar_forward_batchloop_finish",
                "nastar_backward_workspace_bytes", "nastar_backward_replay"))


def load_dev() -> ctypes.CDLL:
    """The DEVELOPMENT build of the search translation unit (``make -C csrc dev``: the A/B switches of csrc/nastar_dev_flags.h -- older
    instruction streams, the compiled step).  Test / probe infrastructure: nothing in the package calls it; ``ops.search_nograd(lib=...)``
    runs a search through it."""
    global _dev_lib
    if _dev_lib is None:
        if not os.path.exists(DEV_LIB_PATH):
            raise NativeLibraryMissing(f"{DEV_LIB_PATH} not found: build it with `make -C {CSRC_DIR} dev`")
        _dev_lib = ctypes.CDLL(DEV_LIB_PATH)
        _bind_search(_dev_lib)
    return _dev_lib


FASTLANE_PATH = os.path.join(_PKG_ROOT, "lib", "_nastar_fastlane.so")
_fastlane = False  # False: not looked for yet; None: absent / switched off


def load_fastlane():
    """(module, address of nastar_forward_ex, address of nastar_placement_from_levels) of the native host lane (csrc/nastar_fastlane.cpp: output allocation, the launch and the poll of
    its completion flag in C++), or None when lib/_nastar_fastlane.so has not been built (`make -C csrc fastlane`) or NASTAR_FASTLANE=0 --
    the Python lane then issues the SAME launch through ctypes (slower on the host, identical on the device)."""
    global _fastlane
    if _fastlane is False:
        _fastlane = None
        if os.environ.get("NASTAR_FASTLANE", "1") != "0" and os.path.exists(FASTLANE_PATH) and not os.environ.get("NASTAR_LIB"):
            import importlib.util
            try:
                spec = importlib.util.spec_from_file_location("_nastar_fastlane", FASTLANE_PATH)
                mod = importlib.util.module_from_spec(spec)
                spec.loader.exec_module(mod)
                fn = ctypes.cast(load().nastar_forward_ex, ctypes.c_void_p).value
                sort_fn = ctypes.cast(load().nastar_placement_from_levels, ctypes.c_void_p).value
                _fastlane = (mod, int(fn), int(sort_fn))
            except Exception as e:  # noqa: BLE001 -- an ABI mismatch of the extension must not take the package down
                import warnings
                warnings.warn(f"neural_astar: {FASTLANE_PATH} could not be loaded ({type(e).__name__}: {e}); using the Python host lane", RuntimeWarning)
    return _fastlane


_levels_entry: dict = {}


def forward_levels_address(H: int, W: int, flags: int) -> int:
    """the address of nastar_forward_levels (include/nastar_levels.h) when a search of H x W maps under ``flags``, without a selection log,
    ranks its levels inside the launch (nastar_levels_in_launch), else 0 -- also 0 when the library lacks the symbol.  Cached per launch
    shape: what the native host lane takes as its trailing ``levels_fn`` argument."""
    key = (H, W, flags)
    v = _levels_entry.get(key)
    if v is None:
        lib = load()
        v = 0
        if hasattr(lib, "nastar_forward_levels") and lib.nastar_levels_in_launch(H, W, flags, 0) == 1:
            v = int(ctypes.cast(lib.nastar_forward_levels, ctypes.c_void_p).value)
        _levels_entry[key] = v
    return v


# NASTAR_EARLY_VERDICT=0 (read once): a checked forward() never returns on the proof of include/nastar_verdict.h -- A/B runs and tests
EARLY_VERDICT = os.environ.get("NASTAR_EARLY_VERDICT", "1") != "0"
_proof_entry: dict = {}


def solvable_proof_address(H: int, W: int) -> int:
    """the address of nastar_solvable_proof (include/nastar_verdict.h) when there is a proof kernel for H x W maps and the early verdict is
    not switched off, else 0 -- also 0 when the library lacks the symbol.  Cached per size: what the native host lane takes as ``proof_fn``."""
    if not EARLY_VERDICT:
        return 0
    v = _proof_entry.get((H, W))
    if v is None:
        lib = load()
        v = 0
        if hasattr(lib, "nastar_solvable_proof") and lib.nastar_solvable_proof_supported(H, W) == 1:
            v = int(ctypes.cast(lib.nastar_solvable_proof, ctypes.c_void_p).value)
        _proof_entry[(H, W)] = v
    return v


_proved_entry: Optional[int] = None


def forward_proved_address() -> int:
    """the address of nastar_forward_proved (include/nastar_ticket.h), or 0 when the library lacks the symbol: what the native host lane takes
    as ``proved_fn`` -- it then issues a search and its proof from that one entry point (whether the proof is ordered by ticket or by event
    is the library's decision, per call)."""
    global _proved_entry
    if _proved_entry is None:
        lib = load()
        _proved_entry = int(ctypes.cast(lib.nastar_forward_proved, ctypes.c_void_p).value) if hasattr(lib, "nastar_forward_proved") else 0
    return _proved_entry


def load() -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeLibraryMissing(
            f"{LIB_PATH} not found: the MI355X HIP extension is the only compute path of this package "
            f"(no CPU fallback). Build it with `make -C {CSRC_DIR}` or `python __graft_entry__.py build`.")
    lib = ctypes.CDLL(LIB_PATH)
    _bind(lib, SIGNATURES)
    _bind(lib, ROUTE_SIGNATURES, ROUTE_SIGNATURES)
    _bind(lib, SOURCE_SIGNATURES, SOURCE_SIGNATURES)
    if hasattr(lib, "nastar_levels_abi"):  # (another build of the C ABI, NASTAR_LIB, may be older than the fourth header)
        _bind(lib, LEVEL_SIGNATURES, LEVEL_SIGNATURES)
    if hasattr(lib, "nastar_fields_abi"):  # (likewise the fifth)
        _bind(lib, FIELD_SIGNATURES, FIELD_SIGNATURES)
    if hasattr(lib, "nastar_fields_tiled_abi"):  # (and the sixth)
        _bind(lib, TILED_FIELD_SIGNATURES, TILED_FIELD_SIGNATURES)
    if hasattr(lib, "nastar_verdict_abi"):  # (and the seventh)
        _bind(lib, VERDICT_SIGNATURES, VERDICT_SIGNATURES)
    if hasattr(lib, "nastar_fields_grad_abi"):  # (and the eighth)
        _bind(lib, FIELD_GRAD_SIGNATURES, FIELD_GRAD_SIGNATURES)
    if hasattr(lib, "nastar_fields_grad_tiled_abi"):  # (and the ninth)
        _bind(lib, FIELD_GRAD_TILED_SIGNATURES, FIELD_GRAD_TILED_SIGNATURES)
    if hasattr(lib, "nastar_field_routes_abi"):  # (and the tenth)
        _bind(lib, FIELD_ROUTE_SIGNATURES, FIELD_ROUTE_SIGNATURES)
    if hasattr(lib, "nastar_path_masks_abi"):  # (and the eleventh)
        _bind(lib, PATH_MASK_SIGNATURES, PATH_MASK_SIGNATURES)
    if hasattr(lib, "nastar_path_masks_tiled_abi"):  # (and the twelfth)
        _bind(lib, PATH_MASK_TILED_SIGNATURES, PATH_MASK_TILED_SIGNATURES)
    if hasattr(lib, "nastar_soft_fields_abi"):  # (and the thirteenth)
        _bind(lib, SOFT_FIELD_SIGNATURES, SOFT_FIELD_SIGNATURES)
    if hasattr(lib, "nastar_soft_fields_tiled_abi"):  # (and the fourteenth)
        _bind(lib, SOFT_FIELD_TILED_SIGNATURES, SOFT_FIELD_TILED_SIGNATURES)
    if hasattr(lib, "nastar_soft_policy_abi"):  # (and the fifteenth)
        _bind(lib, SOFT_POLICY_SIGNATURES, SOFT_POLICY_SIGNATURES)
    if hasattr(lib, "nastar_ticket_abi"):  # (and the sixteenth)
        _bind(lib, TICKET_SIGNATURES, TICKET_SIGNATURES)
    if hasattr(lib, "nastar_soft_policy_tiled_abi"):  # (and the seventeenth)
        _bind(lib, SOFT_POLICY_TILED_SIGNATURES, SOFT_POLICY_TILED_SIGNATURES)
    if hasattr(lib, "nastar_soft_routes_abi"):  # (and the eighteenth)
        _bind(lib, SOFT_ROUTE_SIGNATURES, SOFT_ROUTE_SIGNATURES)
    if hasattr(lib, "nastar_soft_routes_tiled_abi"):  # (and the nineteenth)
        _bind(lib, SOFT_ROUTES_TILED_SIGNATURES, SOFT_ROUTES_TILED_SIGNATURES)
    if hasattr(lib, "nastar_soft_routes_grad_abi"):  # (and the twentieth)
        _bind(lib, SOFT_ROUTES_GRAD_SIGNATURES, SOFT_ROUTES_GRAD_SIGNATURES)
    _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    if rc == NASTAR_OK:
        return
    msg = _ERR_NAMES.get(rc, f"error {rc}")
    if rc == NASTAR_ERR_HIP and _lib is not None:
        msg += ": " + _lib.nastar_last_error().decode("utf-8", "replace")
    raise RuntimeError(f"{what} failed: {msg}")
