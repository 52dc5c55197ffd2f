// Host-only helpers shared by the planners and the launch code: plain C++17, no HIP header, so that a planner header
// (conv_wgrad_plan.h) compiles with any host compiler.  common.h includes this file.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include "../../include/mtdgan_hip.h"

// Lab switches.  The kernel-selection / tuning environment variables of rounds 1-4 (MTD_WINO_*, MTD_WGRAD_*, MTD_IGEMM_*, ...)
// exist only in a library built with -DMTD_LAB (tools/ probes: `MTD_LAB_BUILD=1 python mtd-gan_amd/_build.py --force`).  The
// shipped library reads NO environment variable: a stray MTD_* in a user's shell cannot change which kernel runs.  The few
// options that are meant to be flipped at run time go through mtd_set_option() (api.hip), each exercised by a test.
#ifdef MTD_LAB
static inline const char* mtd_lab_env(const char* name) { return getenv(name); }
#else
static inline const char* mtd_lab_env(const char*) { return nullptr; }
#endif

static inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }
static inline long long geom_pixels(const mtd_geom& g) { return (long long)g.B * g.OH * g.OW; }
