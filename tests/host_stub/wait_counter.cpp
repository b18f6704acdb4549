// Counts the host's waits in a launch-trace library (tests/test_group_knn_cpu.py).  hip_stub_runtime.cpp writes no trace line for
// hipStreamSynchronize, and the trace lines the earlier tests compare must stay what they are: a library linked with
// -Wl,--wrap=hipStreamSynchronize beside this file appends one line "wait" per call to the file BITHTM_STUB_WAITS names (a file of its
// own, not the trace) and goes on to the stub's function.
#include <stdio.h>
#include <stdlib.h>

extern "C" int __real_hipStreamSynchronize(void *stream);

extern "C" int __wrap_hipStreamSynchronize(void *stream) {
    if (const char *path = getenv("BITHTM_STUB_WAITS")) {
        if (FILE *f = fopen(path, "a")) {
            fputs("wait\n", f);
            fclose(f);
        }
    }
    return __real_hipStreamSynchronize(stream);
}
