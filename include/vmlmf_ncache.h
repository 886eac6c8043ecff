/* C ABI of libvmlmf_ncache.so: scoring a text under the language model mixed with a CONTINUOUS CACHE (Model.cache_score,
 * vmlmf_amd/lm.py; Grave, Joulin and Usunier, "Improving Neural Language Models with a Continuous Cache", ICLR 2017) for the AMD
 * Instinct MI355X (gfx950).  A library of its own, loaded on the first cache-scoring call only; one of the Makefile's
 * SIDE.
 *
 * Conventions are vmlmf_contrast.h's: every pointer is a device pointer, every launch goes to `stream` (a hipStream_t passed as
 * void*), nothing synchronises.  Return value: 0 = ok, <0 = VMLMF_E_*, >0 = hipError_t; the text of the last failure of THIS library
 * is vmlmf_ncache_last_error() (thread-local).
 *
 * The cache.  Per batch row it holds pairs (k_j, w_j): k_j the top layer's output behind a token, w_j the token that came next.  A
 * call scores T positions per row against the n pairs carried into it and the pairs of the positions before them in the call: keys
 * (B, L, H) fp32, L = n + T, batch-major, holds the n carried keys of a row, oldest first, and behind them the T outputs of the call
 * itself - row n + t is query t -; key_tok (B, L) int64 holds the tokens that came next, so key_tok[b][n + t] is the target of query t.
 */
#ifndef VMLMF_NCACHE_H
#define VMLMF_NCACHE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VMLMF_NCACHE_ABI_VERSION 1
/* the 16 queries of a workgroup wait in LDS, rows of 16 * ceil(H / 16) + 8 floats: 128.5 KiB of a CU's 160 at this H */
#define VMLMF_NCACHE_MAX_H 2048
/* how many workgroups may share the band of one tile of 16 queries */
#define VMLMF_NCACHE_MAX_PARTS 64

#ifndef VMLMF_E_BADARG
#define VMLMF_E_BADARG (-1)
#define VMLMF_E_WORKSPACE (-4)
#endif

int vmlmf_ncache_abi_version(void);
const char *vmlmf_ncache_last_error(void);

/* Host only.  Bytes of the workspace vmlmf_ncache_score needs: per tile of 16 queries and per tile of 16 keys of the union of its bands
 * three numbers per query, B * ceil(T / 16) * 3 * Wp * 4 with Wp = min(window + 15, n + T) rounded up to a multiple of 16.  0 for sizes
 * vmlmf_ncache_score would refuse. */
size_t vmlmf_ncache_workspace_bytes(int B, int T, int n, int H, int window);

/* Score T positions of B rows under the cache, ONE launch.
 * In:  keys, key_tok as above; vocab_logp (T, B) fp32, time-major: lv, the vocabulary's log-probability of each position's target;
 *      theta (finite) and lam in [0, 1); window >= 1.
 * Per position (t, b), with q = keys[b][n + t], y = key_tok[b][n + t] and the band j in [max(0, n + t - window), n + t) of m pairs:
 *   s_j  = fmul_rn(theta, dot(q, keys[b][j]))
 *   cache_logp[t][b] = log(sum_{j: key_tok[b][j] == y} exp(s_j - M)) - log(sum_j exp(s_j - M)),  M = max_j s_j
 *                      -inf where no band token equals y and where m == 0
 *   logp[t][b]       = logaddexp(log1p(-lam) + lv, log(lam) + cache_logp[t][b])
 *                      log1p(-lam) + lv where cache_logp is -inf;  lv, the same bits, where m == 0 or lam == 0
 * in fp32, the maximum subtracted before every expf.  The order of the sums is fixed by (n, T, window) alone.  Positions go in tiles
 * of 16 (t / 16); the keys of the union of a tile's bands, from jlo = max(0, n + 16 (t / 16) - window), go in tiles of 16.  Per key
 * tile c and query: M_c the maximum of the query's band inside the tile, Z_c = sum expf(s_j - M_c) and N_c the same sum over the
 * matching pairs - a butterfly over the tile's 16 columns, the same values in the same order into both.  Then M = max_c M_c (exact)
 * and Z = sum_c Z_c expf(M_c - M), N = sum_c N_c expf(M_c - M) - 16 lanes, lane l the key tiles l, l + 16, ... of the band in rising
 * order, then a butterfly, the same factors in the same order into both -, cache_logp = logf(N) - logf(Z).  So a band whose every
 * token equals y gives cache_logp 0.0 exactly, and N == 0 exactly where no token matches.  A position's own pair is not in its band.
 * The dot product is fp32 throughout: v_mfma_f32_16x16x4_f32 over H, two accumulators added at the end, an order that depends on H
 * alone.  A workgroup takes (row b, tile of 16 queries, part of the tile's key tiles); parts workgroups share a query tile (0: chosen
 * from B, T, n and window; 1 .. VMLMF_NCACHE_MAX_PARTS: forced).  Each leaves (M_c, Z_c, N_c) of its key tiles in the workspace and
 * takes the query tile's ticket with an agent-scope release; the last to arrive acquires, merges the key tiles and puts the ticket
 * back to zero (ticket: (B * ceil(T / 16)) uint32, zero before the first launch).  Nobody waits for anybody; no floating-point
 * atomics.  The key tiles, not the parts, are the units of the sums: every output is the same bits for every `parts` and from run to
 * run.
 * Nothing outside [0, L) of a row of keys and key_tok is read; nothing but logp, cache_logp, the ticket and the workspace is written.
 * A NaN among the scores of a band makes the position's outputs NaN.
 * Refused with VMLMF_E_BADARG, nothing launched: B, T, H, window < 1; n < 0; B (n + T) >= 2^31; B ceil(T / 16) >= 2^25; H >
 * VMLMF_NCACHE_MAX_H; theta not finite; lam outside [0, 1) or NaN; parts outside [0, VMLMF_NCACHE_MAX_PARTS]; null pointers; keys not
 * 16-byte aligned; workspace not 4-byte aligned.  VMLMF_E_WORKSPACE: workspace_bytes smaller than
 * vmlmf_ncache_workspace_bytes(B, T, n, H, window). */
int vmlmf_ncache_score(int B, int T, int n, int H, int window, float theta, float lam, const float *keys, const int64_t *key_tok,
                       const float *vocab_logp, float *logp, float *cache_logp, uint32_t *ticket, void *workspace,
                       size_t workspace_bytes, int parts, void *stream);

#ifdef __cplusplus
}
#endif
#endif
