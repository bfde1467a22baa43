/*
 * dec_emul_common.h -- what the decoder kernels' translation units (dec_fast_emul.cpp, dec_emul_san.cpp) put in front of the
 * .hip files they include: the host shim, and the two meanings the product's headers leave to an emulation with one thread per
 * lane (ldpc_kernels.h LDPC_DYNAMIC_LDS, ldpc_dec_core.h LDPC_UNIFORM).
 */
#ifndef DEC_EMUL_COMMON_H
#define DEC_EMUL_COMMON_H
#include <hip/hip_runtime.h> /* hip_host/hip/hip_runtime.h: the include path puts it ahead of ROCm's */

/* the launch's dynamic LDS: a heap buffer of exactly lds_bytes, poisoned before every workgroup */
#define LDPC_DYNAMIC_LDS(type, name) HIP_HOST_DYNAMIC_LDS(type, name)
/* readfirstlane: lane 0's value through the wave's exchange slots; one wave barrier, which stands between every lane's code in
 * front of the call and every lane's code behind it (the slots are two sets taken in turn: hip_host_run.h) */
#define LDPC_UNIFORM(x) hip_host_wave_first(x)

/* int32 parameters of dec_emul_decode (ctypes passes one array) */
enum {
  DEC_P_KERNEL, /* 0 fast, 1 fast several-blocks-per-workgroup, 2 fast pull, 3 generic */
  DEC_P_BG,
  DEC_P_Z,
  DEC_P_R,
  DEC_P_SHAPE, /* LDPC_SHAPE_* (fast kernels) */
  DEC_P_N_BLOCKS,
  DEC_P_MAX_ITER,
  DEC_P_OUT_MODE,
  DEC_P_USE_CRC,
  DEC_P_E,
  DEC_P_CRC_TYPE,
  DEC_P_MB,           /* kernel 1: blocks (groups of four) per workgroup; 0: the library's choice for the lifting size */
  DEC_P_JOBS,         /* 1: through job records and the jobs launchers (one job per block, pass counts scattered backwards) */
  DEC_P_PULL_STAGGER, /* kernel 2 */
  DEC_P_PULL_FIRST_ROUND,
  DEC_P_ZC, /* with DEC_P_JOBS, kernel 0: the launcher's zc argument; < 0: the descriptor's lifting size where it has instantiations */
  DEC_P_COUNT
};
/* int32 fields of one job of dec_emul_decode_jobs */
enum { DEC_J_BG, DEC_J_Z, DEC_J_R, DEC_J_MAX_ITER, DEC_J_E, DEC_J_CRC_TYPE, DEC_J_ITER_IDX, DEC_J_ABORT_IDX, DEC_J_COUNT };
/* what dec_emul_fast_info reports of a descriptor */
enum {
  DEC_I_F_OK,
  DEC_I_THREADS,
  DEC_I_LDS,
  DEC_I_NUM_LLR,
  DEC_I_CN_TASKS,
  DEC_I_DOUBLE_TASKS,       /* check-node tasks with f_cn_task[.][0] & 0x100 */
  DEC_I_SHORT_DOUBLE_TASKS, /* ... of which: fewer than 128 items (a thread takes its first item twice) */
  DEC_I_PAIR19,
  DEC_I_EXT_GLOBAL,
  DEC_I_BN_TICKETS,
  DEC_I_BN_TICKET_MAX, /* max f_bn_ticket[.][1]: short tasks grouped into one ticket */
  DEC_I_BN_GROUP,
  DEC_I_MB,
  DEC_I_SUB,
  DEC_I_ZQ,
  DEC_I_GENERIC_THREADS,
  DEC_I_GENERIC_LDS,
  DEC_I_COUNT
};
/* rx_fused_emul_run: int32 fields of one transport block ... */
enum { RXF_T_A, RXF_T_G, RXF_T_BG, RXF_T_QM, RXF_T_NL, RXF_T_RV, RXF_T_ROUND, RXF_T_TBSLBRM, RXF_T_MAX_ITER, RXF_T_LLRLEN /* in and out */,
       RXF_T_C_INIT, RXF_T_COUNT };
/* ... the launch's options ... */
enum {
  RXF_O_LROW,       /* 1: the decoder input lives in LDS when the row fits 160 KiB with the decoder's arrays (tb_api.inc.cpp) */
  RXF_O_MUTE,       /* 1: retransmissions carry LDPC_JOB_MUTE_CHECK */
  RXF_O_ZC,         /* 1: the lifting size's own instantiation when every job has one */
  RXF_O_SCR,        /* 1: the LLRs are a scrambled codeword (the blocks' c_init) */
  RXF_O_INTERLEAVE, /* 1: the jobs of the transport blocks alternate in workgroup order */
  RXF_O_SHAPE,
  RXF_O_TRUNC,      /* 1: first transmissions on the graph cut behind the last column they reach */
  RXF_O_ABORT,      /* 1: the transport blocks' abort flags */
  RXF_O_SYM,        /* 1 (with SCR): each block's input is its symbol record (Qm / 2 planes of G / Qm c16 words), demapped in the prologue */
  RXF_O_COUNT
};
/* ... what it reports of the launch, and per segment */
enum { RXF_I_LROW_OFF, RXF_I_ZC, RXF_I_MUTE, RXF_I_THREADS, RXF_I_LDS, RXF_I_N_SEG, RXF_I_N_CUT, RXF_I_COUNT };
enum { RXF_S_ITER, RXF_S_NUM_LLR, RXF_S_Z, RXF_S_NCORE, RXF_S_TB, RXF_S_COUNT };
#endif
