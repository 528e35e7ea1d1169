/* host_check.h — what the stand-alone *_host_check programs share: the last-error stub the rtr_*_host.cpp link against outside the
 * library, the random numbers of their inputs, exactly sized 16-B aligned arrays, and the count of refusals.  Included once per program. */
#pragma once
#include "../rtr_arg_check.h"

#include <cstdio>
#include <cstdlib>
#include <string>

static std::string g_err;
void rtrdev::set_last_error(const char* msg) { g_err = msg; }

static uint32_t lcg(uint32_t& s) { s = s * 1664525u + 1013904223u; return s; }
static float unit(uint32_t& s) { return (float)(lcg(s) >> 8) * (1.0f / 16777216.0f); }

template <class T>
static T* aligned(size_t n) { return static_cast<T*>(aligned_alloc(16, (n * sizeof(T) + 15) / 16 * 16)); }

/* 0 when rc is a refusal whose message starts with who and names needle */
static int expect_refused(int rc, const char* who, const char* needle) {
    if (rc == RTR_ERR_INVALID_ARGUMENT && g_err.find(std::string(who) + ": ") == 0 && g_err.find(needle) != std::string::npos) return 0;
    fprintf(stderr, "expected a refusal of %s naming '%s', got %d '%s'\n", who, needle, rc, g_err.c_str());
    return 1;
}

/* in a scope with the counters `bad` and `refusals` */
#define REFUSED(call, who, needle) do { bad += expect_refused(call, who, needle); ++refusals; } while (0)
