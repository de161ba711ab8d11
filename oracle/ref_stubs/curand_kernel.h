/*
 * curand_kernel.h -- TEST INFRASTRUCTURE: a host stand-in for cuRAND's device API.  curandState does not generate
 * anything: it REPLAYS the sequence its owner queued with curand_replay() before the call, so that a test harness
 * decides every "random" number a kernel draws (uniforms in (0, 1], as curand_uniform returns them).  Once the queue is
 * empty every draw returns 0.5.  curand_init() leaves the queue alone.
 */
#ifndef RT_STUB_CURAND_KERNEL_H
#define RT_STUB_CURAND_KERNEL_H

#include "cuda_runtime.h"

struct curandState { int unused; };

inline float curand_replay_queue[64];
inline int curand_replay_n = 0, curand_replay_at = 0, curand_replay_drawn = 0;

static inline void curand_replay(const float *seq, int n) {
    curand_replay_n = n < 64 ? n : 64;
    for (int i = 0; i < curand_replay_n; i++) curand_replay_queue[i] = seq[i];
    curand_replay_at = 0;
    curand_replay_drawn = 0;
}
static inline void curand_init(unsigned long long, unsigned long long, unsigned long long, curandState *) {}
static inline float curand_uniform(curandState *) {
    curand_replay_drawn++;
    return curand_replay_at < curand_replay_n ? curand_replay_queue[curand_replay_at++] : 0.5f;
}

#endif
