// extern_parse_host.cpp -- the product's timestamp() / ip() parse definitions (timeparse.h,
// netparse.h: the text the device packer compiles) as a stand-alone host program, built by
// tests/test_rfc3339_independent.py with AddressSanitizer and UBSan.
//
// stdin:  one string per line, hex-encoded (an empty line is the empty string).
// stdout: one line per string:  <ts ok> <sec> <nsec> <ip ok> <32 hex digits of the 16-byte form>
//
// Every string is parsed from a heap buffer of exactly its length: the device's string blob carries
// slack bytes behind the last string that would hide a read past the end, this buffer has none.
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include <memory>
#include <string>

#include "timeparse.h"

static int hexval(int c) {
    if (c >= '0' && c <= '9') return c - '0';
    if (c >= 'a' && c <= 'f') return c - 'a' + 10;
    return -1;
}

int main() {
    std::string line;
    int c;
    bool more = true;
    while (more) {
        line.clear();
        while ((c = getchar()) != EOF && c != '\n') line.push_back((char)c);
        if (c == EOF) {
            if (line.empty()) break;
            more = false;
        }
        if (line.size() % 2) {
            fprintf(stderr, "odd hex line\n");
            return 2;
        }
        const size_t n = line.size() / 2;
        std::unique_ptr<uint8_t[]> s(new uint8_t[n]);  // exact size: no byte behind the string
        for (size_t i = 0; i < n; i++) {
            const int hi = hexval(line[2 * i]), lo = hexval(line[2 * i + 1]);
            if (hi < 0 || lo < 0) {
                fprintf(stderr, "bad hex line\n");
                return 2;
            }
            s[i] = (uint8_t)(hi * 16 + lo);
        }
        int64_t sec = 0;
        int32_t nsec = 0;
        const bool tok = mxptime::parse_rfc3339(s.get(), n, &sec, &nsec);
        uint8_t ip[16];
        memset(ip, 0, sizeof ip);
        const bool iok = mxpnet::parse_ip(s.get(), (uint32_t)n, ip);
        printf("%d %" PRId64 " %d %d ", tok ? 1 : 0, tok ? sec : 0, tok ? nsec : 0, iok ? 1 : 0);
        for (int k = 0; k < 16; k++) printf("%02x", iok ? ip[k] : 0);
        printf("\n");
    }
    return 0;
}
