// Force-included in front of the reference's Scene.cpp (TEST INFRASTRUCTURE): rand() and RAND_MAX of the Microsoft C runtime the
// reference was built with, unseeded. The constants are the ones cuda-path-tracer-ss_amd/host/Scene.cpp states (Scene::nextRand).
#pragma once
// every standard header that names rand itself comes first, so that the macro below reaches the reference's text only
#include <algorithm>
#include <cstdlib>
#include <random>
#include <stdlib.h>
extern unsigned int ref_rand_state;   // ref_probe.cpp; 1 = the C runtime's state before any srand()
inline int ref_msvc_rand() {
    ref_rand_state = ref_rand_state * 214013u + 2531011u;
    return (int)((ref_rand_state >> 16) & 0x7fffu);
}
#undef RAND_MAX
#define RAND_MAX 32767
#define rand ref_msvc_rand
