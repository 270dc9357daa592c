// What the sources of the TEST-ONLY library libfawkes_fieldtest.so share (fieldtest.hip, fieldtest_tower.hip): the return codes, the
// error state and the one way a batch of cases goes to the device and back.  Not part of the product.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace ft {

enum { FT_OK = 0, FT_BAD_ARGUMENT = 1, FT_HIP_ERROR = 2, FT_AFTER_ERROR = 3 };

extern char g_err[512];
extern bool g_failed;       // after a HIP error nothing more is launched, by any entry point of the library

// records the message for ft_last_error() and returns `code`
int fail(int code, const char *what, const char *detail);

// `bin` bytes in, `bout` bytes out (0xee-filled before the launch: a result nobody wrote is not a valid one), launch(din, dout) in
// between, synchronous on device 0.  Returns a code, never aborts; the buffers are left alone after an error.
template <class Launch>
int device_run(const void *in, size_t bin, void *out, size_t bout, Launch launch) {
    if (g_failed) return FT_AFTER_ERROR;
    uint32_t *din = nullptr, *dout = nullptr;
    hipError_t e = hipSetDevice(0);
    const char *step = "hipSetDevice";
    if (e == hipSuccess) { step = "hipMalloc"; e = hipMalloc((void **)&din, bin); }
    if (e == hipSuccess) e = hipMalloc((void **)&dout, bout);
    if (e == hipSuccess) { step = "hipMemcpy (to device)"; e = hipMemcpy(din, in, bin, hipMemcpyHostToDevice); }
    if (e == hipSuccess) { step = "hipMemset"; e = hipMemset(dout, 0xee, bout); }
    if (e == hipSuccess) {
        step = "kernel launch";
        launch(din, dout);
        e = hipGetLastError();
    }
    if (e == hipSuccess) { step = "hipDeviceSynchronize"; e = hipDeviceSynchronize(); }
    if (e == hipSuccess) { step = "hipMemcpy (to host)"; e = hipMemcpy(out, dout, bout, hipMemcpyDeviceToHost); }
    if (e != hipSuccess) return fail(FT_HIP_ERROR, step, hipGetErrorString(e));
    (void)hipFree(din);
    (void)hipFree(dout);
    return FT_OK;
}

}  // namespace ft
