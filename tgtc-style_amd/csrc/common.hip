#include "common.h"

namespace tgtc {

char* err_buf() {
    static thread_local char buf[512] = "";
    return buf;
}

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err_buf(), 512, fmt, ap);
    va_end(ap);
    return code;
}

int cu_count(int& cus) {
    int dev = 0;
    TGTC_HIP_CHECK(hipGetDevice(&dev));
    TGTC_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    return TGTC_OK;
}

}  // namespace tgtc

extern "C" int tgtc_version(void) { return 101; /* 0.1.1: explicit render path (tgtc_render_path) */ }
extern "C" const char* tgtc_last_error(void) { return tgtc::err_buf(); }
