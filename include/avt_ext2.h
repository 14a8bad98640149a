/*
 * avt_ext2.h — second extension header of the C ABI (include/avt.h holds the pinned table, include/avt_ext.h the first
 * extension: their conventions, status codes and declaration grammar apply here unchanged, and the ctypes binding reads all
 * three headers with the same parser).  No name declared here is declared in either of the other two.
 *
 * Extension 2, version 1: the training state — parameters, buffers, momentum buffers — copied between its tensors and ONE
 * flat device buffer in one launch, so that an epoch-end checkpoint costs the training stream one kernel and one
 * device-to-host copy instead of one copy per tensor.
 */
#ifndef AVT_EXT2_H
#define AVT_EXT2_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AVT_EXT2_VERSION 1  /* 1: the one-launch state copy */

/* HOST.  AVT_EXT2_VERSION of the library. */
int avt_ext2_version(void);

/* A byte-granular copy of many tensors in one launch (csrc/state_copy.hip).  The job-table pattern of avt_sgd_multi and
 * avt_grad_pack_multi (avt.h): `jobs` a DEVICE array of AvtStateJob, `blk2job` a DEVICE int32 [nblocks]; job j owns blocks
 * blk0 .. blk0 + ceil(nbytes / 16384), block b the bytes [(b - blk0) * 16384, + 16384) of its job (64-bit offsets).
 * dst[i] = src[i] for 0 <= i < nbytes; nothing outside [dst, dst + nbytes) is written.  Where src | dst is 16-byte aligned a
 * lane moves 16 bytes per access, where it is 4-byte aligned a dword, otherwise single bytes; the nbytes % 16 and nbytes % 4
 * tails take the narrower access.  src and dst of one job must not overlap; the jobs' destinations must not overlap each
 * other.  The same entry packs (tensors -> flat buffer) and unpacks (flat buffer -> tensors): only the table differs.  The
 * caller validates the jobs (dense tensors, the flat buffer's slots); avt_state_job_bytes() = sizeof(AvtStateJob) = 32.
 * AVT_ERR_ARG before any launch for a NULL pointer, nblocks <= 0, a job table that is not 8-byte aligned or a block map that
 * is not 4-byte aligned. */
typedef struct AvtStateJob {
  const void* src;
  void* dst;
  int64_t nbytes;
  int32_t blk0;          /* first block of the job in the launch */
  int32_t pad;
} AvtStateJob;
int avt_state_job_bytes(void);
int avt_state_copy_multi(const void* jobs, const int32_t* blk2job, int nblocks, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AVT_EXT2_H */
