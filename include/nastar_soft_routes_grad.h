/* nastar_soft_routes_grad.h -- the SCORE-FUNCTION backward of the sampled routes of include/nastar_soft_routes.h: the gradient, with respect
 * to the cost maps, of sum over the walkers of g * log p(route), for an upstream gradient g of log_prob_out.  What REINFORCE needs: the
 * routes are samples, not functions of the costs, and log p is.  A twentieth header BESIDE the others: nothing in them changes,
 * NASTAR_VERSION stays what it is -- ask nastar_soft_routes_grad_abi().
 *
 * log p(route) = (V_K(n_0) - cost(route)) / tau, and cost(route) is the sum of cost over every route cell but the last, so
 *
 *     d log p(route) / d cost = (dV_K(n_0) / d cost - visits(route)) / tau
 *
 * The first term is the vector-Jacobian product nastar_soft_fields_backward computes from the forward's tape, for a grad_dist that holds the
 * walkers' g summed at their start cells; the second is a histogram of the routes the walkers wrote, weighted with g.  Both sums over
 * walkers are taken in FIXED POINT: sums of integers, exact and order-free, so the result is a pure function of the inputs -- the same
 * bits from two calls, from any split of the walkers over workgroups and from either kernel shape of the walkers' launch -- and no
 * floating-point atomic is used.
 *
 * Per call: the maps, neighbor_mask, tau, horizon K and tape of the nastar_soft_cost_to_go call; start_idx [B,S]; routes [B,S,N,route_cap],
 * route_len [B,S,N] and status [B,S] exactly as nastar_soft_routes wrote them (rows of at least K + 1 cells: the whole route from the
 * start on); grad_log_prob [B,S,N] fp32, g below.
 *
 *   ok         a walker (b, s, i) is ok when status[b,s] == 0.  The g of a walker that is not ok is NEVER READ: a NaN or an infinity there
 *              reaches no output (the rule of the live cells of nastar_soft_fields.h).
 *   scale      per map, M_b = the largest |g| over its ok walkers and e_b = ilogb(M_b) (the exponent of a subnormal M_b counted as of a
 *              normal number: 2^e_b <= M_b < 2^(e_b + 1)).  P = min(40, 61 - ceil(log2(S * N * K))).  A call with P < 30 is refused.
 *   q          q(b,s,i) = llrint(ldexp((double)g, P - e_b)): g in units of 2^(e_b - P), rounded to nearest, ties to even.
 *              |q| <= 2^(P + 1).
 *   Q_visit    [b,n] int64: the sum, over the ok walkers of map b and over every route cell BUT THE LAST that equals n, of q.  A cell a route
 *              stands on twice counts twice.  A row entry outside [0, H*W) is skipped and route_len is read as min(route_len, K + 1):
 *              nothing the caller passes moves a store out of the planes.
 *   Q_seed     [b,n] int64: the sum of q over the ok walkers of map b with start_idx[b,s] == n.
 *   overflow   a route has at most K cells but the last, so |Q_visit| <= S*N*K * 2^(P + 1) <= 2^ceil(log2(S*N*K)) * 2^(P + 1) <=
 *              2^(61 - P) * 2^(P + 1) = 2^62 < 2^63, and |Q_seed| <= S*N * 2^(P + 1) is smaller: no sum leaves int64.
 *   seed       seed[b,n] = (float)((double)Q_seed[b,n] * 2^(e_b - P)).
 *   A32        nastar_soft_fields_backward of the seed plane as grad_dist: the existing kernel and its bits.  It reads the seed on the
 *              cells live at K only, which drops the seeds of goal starts: a walker that starts on a goal contributes nothing.
 *   output     grad_cost_out[b,n] = (float)(((double)A32[b,n] - (double)Q_visit[b,n] * 2^(e_b - P)) / tau): fp64 throughout, rounded once
 *              at the store.
 *   special    a map with M_b == 0 or without an ok walker: every cell 0.0f.  A map where the g of an ok walker is not finite: every
 *              cell NaN (the other maps are unaffected).
 *   status_out per map, int32: NASTAR_ERR_BAD_COST (9, the forward's rule) and an all-zero gradient, else NASTAR_OK.
 *
 * How: at most five launches on `stream`, nothing is read back, so the call can be captured into a graph.  (1) per map, M_b and the
 * non-finite flag, and the zeros of the two int64 planes; (2) the histogram: one wavefront per walker reads its row, 64 cells a round, and
 * adds q with 64-bit INTEGER atomics into an int64 plane of the map in LDS, whose non-zero cells the workgroup then adds to the plane in
 * device memory, again with 64-bit integer atomics; (3) the seed plane; (4) nastar_soft_fields_backward's launch; (5) the output.
 */
#ifndef NASTAR_SOFT_ROUTES_GRAD_H_
#define NASTAR_SOFT_ROUTES_GRAD_H_

#include "nastar_soft_routes.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NASTAR_SOFT_ROUTES_GRAD_ABI 1

/* 1: the definition above */
int nastar_soft_routes_grad_abi(void);

/* the largest H*W nastar_soft_routes_backward takes: nastar_soft_fields_grad_max_cells() (6144), the limit of the field's backward */
int nastar_soft_routes_grad_max_cells(void);

/* the bytes of the workspace of a call: two int64 planes and two fp32 planes of B * H * W cells and the scale of every map; 0 when an
 * argument is below 1, SIZE_MAX when the product does not fit */
size_t nastar_soft_routes_grad_workspace_bytes(int B, int H, int W);

/* cost, goal, passable: [B,H,W] fp32, device; tape, tape_bytes, neighbor_mask, tau, horizon: those of the nastar_soft_cost_to_go call;
 * start_idx [B,S] int32; routes [B,S,N,route_cap] int32, route_len [B,S,N] int32, status [B,S] int32: what nastar_soft_routes wrote;
 * grad_log_prob [B,S,N] fp32; grad_cost_out [B,H,W] fp32; status_out [B] int32; workspace: device memory of workspace_bytes >=
 * nastar_soft_routes_grad_workspace_bytes(B, H, W) bytes, 16-byte aligned.  Enqueued on `stream`, no host read.  Refused before any HIP
 * call, in this order: an invalid neighbor_mask (NASTAR_ERR_UNSUPPORTED); a NULL cost / goal / passable / tape / start_idx / routes /
 * route_len / status / grad_log_prob / grad_cost_out / status_out (NASTAR_ERR_NULL); B, S, N, H, W or horizon < 1, a tau that is not
 * finite and positive, or route_cap < horizon + 1 -- the backward reads whole rows and does not replay walks -- (NASTAR_ERR_BAD_SHAPE);
 * H*W above nastar_soft_routes_grad_max_cells(), B*S*N above 2^30, or P < 30 (NASTAR_ERR_UNSUPPORTED); a tape or a workspace that is
 * missing, too small or misaligned (NASTAR_ERR_WORKSPACE).  After a HIP error nothing more is enqueued and NASTAR_ERR_HIP is returned. */
int nastar_soft_routes_backward(const float* cost, const float* goal, const float* passable, const void* tape, size_t tape_bytes,
                                const int32_t* start_idx, const int32_t* routes, int route_cap, const int32_t* route_len,
                                const int32_t* status, const float* grad_log_prob, int B, int S, int N, int H, int W, unsigned neighbor_mask,
                                double tau, int horizon, float* grad_cost_out, int32_t* status_out, void* workspace, size_t workspace_bytes,
                                void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NASTAR_SOFT_ROUTES_GRAD_H_ */
