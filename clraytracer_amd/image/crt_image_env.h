// crt_image_env.h -- the environment switches of the image libraries that have measured choices (libcrt_denoise.so, libcrt_temporal.so,
// libcrt_vfilter.so): read by every call, and anything but a listed value means the measured default. libcrt_motion.so has no switch and does
// not include this file.
#pragma once
#include <stdlib.h>
#include <string.h>

// the largest step whose taps come from LDS: NAME=0|1|2|4
static inline int crti_env_step(const char* name, int deflt)
{
    const char* e = getenv(name);
    if (e && e[0] && !e[1] && (e[0] == '0' || e[0] == '1' || e[0] == '2' || e[0] == '4')) return e[0] - '0';
    return deflt;
}

// one of two words: NAME=off|on
static inline bool crti_env_choice(const char* name, const char* off, const char* on, bool deflt)
{
    const char* e = getenv(name);
    if (e && !strcmp(e, on)) return true;
    if (e && !strcmp(e, off)) return false;
    return deflt;
}
