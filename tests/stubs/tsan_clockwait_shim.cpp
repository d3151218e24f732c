/*
 * tsan_clockwait_shim.cpp — linked into the thread-sanitizer build of batcher_soak only (tests/stubs/Makefile).
 *
 * std::condition_variable::wait_for on the steady clock (the scheduler's wait for expected owners) calls pthread_cond_clockwait.  The thread
 * sanitizer runtime of GCC 11 has no interceptor for that call, so it never sees the mutex released and retaken inside the wait: it then reports a
 * "double lock" and a false race for everything the mutex guards.  This definition, which the program's own symbol table puts in front of the C
 * library's, turns the call into pthread_cond_timedwait, which the runtime does intercept.  With a runtime that knows the call the shim is harmless.
 */
#include <pthread.h>
#include <time.h>

extern "C" int pthread_cond_clockwait(pthread_cond_t* cond, pthread_mutex_t* mutex, clockid_t clock, const struct timespec* abstime) {
    struct timespec now_c, now_r, abs_r;
    clock_gettime(clock, &now_c);
    clock_gettime(CLOCK_REALTIME, &now_r);
    long long ns = (abstime->tv_sec - now_c.tv_sec) * 1000000000ll + (abstime->tv_nsec - now_c.tv_nsec);
    if (ns < 0) ns = 0;
    ns += now_r.tv_sec * 1000000000ll + now_r.tv_nsec;
    abs_r.tv_sec = (time_t)(ns / 1000000000ll);
    abs_r.tv_nsec = (long)(ns % 1000000000ll);
    return pthread_cond_timedwait(cond, mutex, &abs_r);
}
