// amg_host.h — what a host-only unit needs from libamg.so: the public header and the error plumbing, no HIP header.
#pragma once
#include <cstdint>
#include <string>

#include "../../include/amg.h"

// ------------------------------------------------------------------ error plumbing
extern thread_local std::string g_amg_err;
int amg_fail(int code, const char* fmt, ...);
