// What the stand-alone host-check programs (tools/*_host_check.cpp) share: the EXPECT macro, the failure count, the buffers that stand in
// for device arrays and the closing "<name>: ok" line.  A program defines HOST_CHECK_NAME before it includes this.
#pragma once
#include <stdio.h>
#include <string.h>

#include "../include/neurovit_hip.h"

extern "C" const char* nv_last_error(void);

static int failures = 0;
#define EXPECT(cond)                                                                                  \
  do {                                                                                                \
    if (!(cond)) {                                                                                    \
      printf(HOST_CHECK_NAME ": FAILED %s (line %d): %s\n", #cond, __LINE__, nv_last_error());         \
      ++failures;                                                                                     \
    }                                                                                                 \
  } while (0)

// Nothing is launched, so no call reads or writes through these; the sanitizers watch their ends all the same.
alignas(16) [[maybe_unused]] static float f[64] = {0};
[[maybe_unused]] static int idx[64] = {0};

static int host_check_result() {
  if (failures) return 1;
  printf(HOST_CHECK_NAME ": ok\n");
  return 0;
}
