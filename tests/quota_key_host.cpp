// quota_key_host.cpp -- the value formatter of memquota's makeKey (istio_amd/csrc/quota_key_fmt.h:
// the text the device's key stage compiles) as a stand-alone host program, built by
// tests/test_quota_key_fmt.py with AddressSanitizer and UBSan.
//
// stdin:  one value per line: <kind> <16 hex digits of the value's 64 bits>
// stdout: one line per value: the formatted bytes, hex-encoded
//
// Every value is formatted into a heap buffer of exactly mxp_qk_len bytes: a byte more than the
// length pass promised is a heap overflow the sanitizer reports, a byte less is reported here.
#include <inttypes.h>
#include <stdio.h>

#include <memory>

#include "quota_key_fmt.h"

struct Sink {
    uint8_t* p;
    uint32_t at;
    void operator()(uint8_t b) { p[at++] = b; }
};

int main() {
    unsigned kind;
    uint64_t bits;
    while (scanf("%u %" SCNx64, &kind, &bits) == 2) {
        if (kind != MXP_QK_INT64 && kind != MXP_QK_DOUBLE && kind != MXP_QK_BOOL) {
            fprintf(stderr, "bad kind %u\n", kind);
            return 2;
        }
        const uint32_t n = mxp_qk_len(kind, bits);
        std::unique_ptr<uint8_t[]> buf(new uint8_t[n]);  // exact size
        Sink s{buf.get(), 0};
        mxp_qk_fmt(kind, bits, s);
        if (s.at != n) {
            fprintf(stderr, "kind %u bits %016" PRIx64 ": %u bytes written, %u counted\n", kind, bits, s.at, n);
            return 3;
        }
        for (uint32_t i = 0; i < n; i++) printf("%02x", buf[i]);
        printf("\n");
    }
    return 0;
}
