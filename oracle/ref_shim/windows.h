/*
 * Stand-in <windows.h> for building the reference speechPlayer sources on Linux (oracle/Makefile, target `ref`).
 * TEST INFRASTRUCTURE ONLY; this project's own text.  It supplies exactly what the reference's lock.h and
 * speechPlayer.cpp / speechWaveGenerator.cpp take from the Windows SDK: CRITICAL_SECTION (re-entrant for its owner),
 * InterlockedIncrement / InterlockedDecrement, and the min / max macros.
 */
#pragma once
/* every standard header the reference includes AFTER this one, before min / max become macros */
#include <pthread.h>
#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <list>
#include <queue>

typedef pthread_mutex_t CRITICAL_SECTION;

static inline void InitializeCriticalSection(CRITICAL_SECTION *cs)
{
    pthread_mutexattr_t attr;
    pthread_mutexattr_init(&attr);
    pthread_mutexattr_settype(&attr, PTHREAD_MUTEX_RECURSIVE);
    pthread_mutex_init(cs, &attr);
    pthread_mutexattr_destroy(&attr);
}
static inline void DeleteCriticalSection(CRITICAL_SECTION *cs) { pthread_mutex_destroy(cs); }
static inline void EnterCriticalSection(CRITICAL_SECTION *cs) { pthread_mutex_lock(cs); }
static inline void LeaveCriticalSection(CRITICAL_SECTION *cs) { pthread_mutex_unlock(cs); }
static inline long InterlockedIncrement(volatile long *p) { return __sync_add_and_fetch(p, 1); }
static inline long InterlockedDecrement(volatile long *p) { return __sync_sub_and_fetch(p, 1); }

#define max(a, b) (((a) > (b)) ? (a) : (b))
#define min(a, b) (((a) < (b)) ? (a) : (b))

/* The reference draws its noise from the process-global rand(); the build sends those calls to ref_noise.cpp instead. */
extern "C" int ref_rand(void);
#define rand ref_rand
