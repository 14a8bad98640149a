/*
 * avt_ext.h — extension entries of the C ABI (include/avt.h holds the pinned table: its conventions, status codes and
 * declaration grammar apply here unchanged, and the ctypes binding reads both headers with the same parser).
 *
 * Extension 1: the DETERMINISTIC weight gradients of the training step.  The entries of avt.h split the reduction over
 * output positions across workgroups and add the partial tiles into dW with fp32 atomics, so the summation order — and
 * with it the last bits of dW — changes from run to run.  The entries below compute the same partial tiles with the same
 * arithmetic, but a workgroup STORES its tile into a workspace slot that depends on its (chunk, tile) indices alone, and a
 * second launch on the same stream sums the chunks in ascending order in fp32 and WRITES dW (no zeroing, nothing
 * accumulated).  No workgroup waits for another; the split into chunks is computed on the host from the shapes alone.
 * Same inputs + same build -> the same bits, on one device.
 */
#ifndef AVT_EXT_H
#define AVT_EXT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AVT_EXT_VERSION 1  /* 1: the deterministic weight gradients */

/* HOST.  AVT_EXT_VERSION of the library. */
int avt_ext_version(void);

/* HOST.  Bytes of workspace avt_conv3d_wgrad_x3_det_sub_f32 needs for this geometry (the arguments of that entry that
 * decide it): chunks * cout * taps * cin * 4.  0 for a geometry that entry refuses (avt_last_error says why). */
int64_t avt_conv3d_wgrad_x3_det_ws_bytes(int batch, int t, int h, int w, int cin, int cout, int kt, int kh, int kw, int st,
                                         int sh, int sw, int pt, int ph, int pw, int to, int ho, int wo, int ldx, int ldy,
                                         int ldw);
/* avt_conv3d_wgrad_x3_sub_f32 (avt.h) with a fixed summation order: the same arguments without zero_dw — dW's E = taps * cin
 * columns of each of its cout rows (ldw elements apart; 0 = E) are WRITTEN, columns beyond E are left alone, so the frame-tap
 * slices of a longer filter are independent calls.  Always the phase-serial tile (128 x {128, 64, 32}; buffer loads as
 * avt_wgrad_x3_set_xl(5 / 6) says).  ws: device memory, 16-byte aligned, at least avt_conv3d_wgrad_x3_det_ws_bytes(...)
 * bytes, contents arbitrary on entry, owned by the call until the stream has run it; every byte read from it was written
 * by this call.  AVT_ERR_ARG before any launch for a NULL, misaligned or short workspace and for everything the atomic
 * entry refuses. */
int avt_conv3d_wgrad_x3_det_sub_f32(const float* dy, const float* x, float* dw, int batch, int t, int h, int w, int cin,
                                    int cout, int kt, int kh, int kw, int st, int sh, int sw, int pt, int ph, int pw, int to,
                                    int ho, int wo, int ldx, int ldy, int ldw, void* ws, int64_t ws_bytes, void* stream);

/* HOST.  Launches so far, in this process, of the deterministic tile form (bn = 32 / 64 / 128 outputs on the shorter axis; swap: 1 =
 * cout on the 128-wide axis; buf: 1 = buffer loads): what tests assert their coverage of the forms with.  -1: no such form. */
int64_t avt_conv3d_wgrad_x3_det_launches(int bn, int swap, int buf);

/* HOST.  Bytes of workspace avt_stem_wgrad_x3_det needs: workgroups-per-slice * cout * kt * 7 * 32 * 4.  0 for a shape that
 * entry refuses. */
int64_t avt_stem_wgrad_x3_det_ws_bytes(int batch, int t, int h, int pw, int cout, int kt, int pt);
/* avt_stem_wgrad_x3 (avt.h) with a fixed summation order: a workgroup's eight waves meet in the LDS in ordered rounds
 * (column block 0 stores, barrier, block 1 adds, ...), the workgroups' partial filters go to the workspace and are summed
 * in ascending workgroup order.  dw[cout][kt][7][4][8] is WRITTEN: the caller does not zero it.  ws as above.  Shapes as
 * avt_stem_wgrad_x3_supported, less kt = 5 with cout != 8 (that instance's staging area does not fit a CU's LDS: refused here
 * with AVT_ERR_ARG instead of failing at the launch). */
int avt_stem_wgrad_x3_det(const void* x_hi, const void* x_lo, const float* dy, float* dw, int batch, int t, int h, int pw,
                          int cout, int kt, int pt, void* ws, int64_t ws_bytes, void* stream);

/* HOST.  Launches so far of the deterministic stem instance (kt 1 / 5; co = 8, or 16 for every multiple of 16).  -1: no such instance. */
int64_t avt_stem_wgrad_x3_det_launches(int kt, int co);

#ifdef __cplusplus
}
#endif
#endif /* AVT_EXT_H */
