/* rrnet_hip_attn.h — companion header of rrnet_hip.h: the dilated-window attention of modules/self_attention.py
 * (csrc/attn.hip), exported by the same librrnet_hip.so.  Same conventions as rrnet_hip.h: C ABI, 0 on success,
 * rr_last_error() holds the message of a failure, every entry enqueues on `stream` and returns; pointers are device
 * pointers.  rrnet_amd/_C.py types the bindings from this file with the parser it uses for rrnet_hip.h (_C.Family). */
#ifndef RRNET_HIP_ATTN_H
#define RRNET_HIP_ATTN_H

#ifdef __cplusplus
extern "C" {
#endif

#ifndef __HIP_INCLUDE_HIP_HIP_RUNTIME_API_H__
#ifndef RRNET_HIP_H
typedef struct ihipStream_t *hipStream_t;
#endif
#endif

/* ---- dilated-window attention (attn.hip) ------------------------------------------------------------------------ *
 * modules/self_attention.py:67-91 without the unfolded tensors.  q, k [n, h, w, ck], v [n, h, w, cv], NHWC fp32; window
 * (kh, kw), dilation (dh, dw), padding (ph, pw), stride 1; T = kh * kw taps, tap t = a * kw + b.
 *   oh = h + 2 ph - dh (kh - 1), ow = w + 2 pw - dw (kw - 1); centre cy = dh (kh / 2) - ph, cx = dw (kw / 2) - pw.
 *   output (i, j), tap (a, b) reads the source (y, x) = (i - ph + a dh, j - pw + b dw);
 *   logit[t] = q[i + cy, j + cx, :] . k[y, x, :] inside the map, 0 outside (F.unfold pads with zeros: a padded tap is
 *   NOT masked, it enters the softmax with logit 0 and value 0); P = softmax_t(logit), maximum subtracted;
 *   ctx[i, j, :] = sum over the taps inside of P[t] v[y, x, :].
 * rr_attn_fwd: ctx [n, oh, ow, cv] and the stashed p [n, oh, ow, T].
 * rr_attn_bwd_q: dP[t] = dctx[i, j, :] . v[y, x, :] (0 outside), ds = P (dP - sum_t P dP) -> ds [n, oh, ow, T];
 *   dq [n, h, w, ck] written whole: dq[i + cy, j + cx, :] = sum over the taps inside of ds[t] k[y, x, :], 0 at the
 *   query positions no output reads.
 * rr_attn_bwd_kv: gather over the (i, j, t) that read (y, x), taps ascending: dk[y, x, :] = sum ds[i, j, t] q[i + cy, j + cx, :],
 *   dv[y, x, :] = sum p[i, j, t] dctx[i, j, :]; both written whole.
 * No floating-point atomics, every sum has a fixed order.  Refused (status, no launch): a null pointer, ck % 4 or cv % 4,
 * cy < 0 or cx < 0, oh < 1 or ow < 1, cy + oh > h or cx + ow > w (outputs without a query: the reference cannot
 * broadcast them either), T > 64. */
int rr_attn_fwd(const float *q, const float *k, const float *v, float *ctx, float *p, int n, int h, int w, int ck, int cv,
                int kh, int kw, int dh, int dw, int ph, int pw, hipStream_t stream);
int rr_attn_bwd_q(const float *dctx, const float *v, const float *k, const float *p, float *ds, float *dq, int n, int h, int w,
                  int ck, int cv, int kh, int kw, int dh, int dw, int ph, int pw, hipStream_t stream);
int rr_attn_bwd_kv(const float *ds, const float *p, const float *q, const float *dctx, float *dk, float *dv, int n, int h, int w,
                   int ck, int cv, int kh, int kw, int dh, int dw, int ph, int pw, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RRNET_HIP_ATTN_H */
