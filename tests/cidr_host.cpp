// cidr_host.cpp -- the host half of the product's IP_ADDRESSES list (istio_amd/csrc/cidr.h: addEntry
// on ParseCIDR, the merged interval tables, the /16 directory) as a stand-alone host program, built
// by tests/test_cidr_independent.py with AddressSanitizer and UBSan.  mxp_list_create needs a GPU;
// this program runs the same text without one.
//
// stdin: lines of one tag byte and a hex-encoded string (nothing after the tag: the empty string):
//   e<hex>  a list entry          o<hex>  an override          l<hex>  a lookup
//   =       end of one list: its output is printed and the next list starts
// stdout, per list, in this order:
//   E <0|1>          per entry, in order: ParseCIDR refused / accepted it
//   O <0|1>          per override, likewise
//   N <n>            numEntries: accepted entries + accepted overrides
//   4 <lo> <hi>      per IPv4 interval of the merged table (decimal)
//   6 <lo> <hi>      per IPv6 interval (32 hex digits each)
//   D <k> <value>    the 65,537 directory values as their runs: k = 0, and every k whose value
//                    differs from the one at k - 1 (lossless: the test expands it again)
//   L <-1|0|1>       per lookup: mxpnet::parse_ip, then a plain linear scan of the tables above
//   =
// Unlike mxp_list_create this goes on after a refused entry, so one run reports every entry.
//
// Every string is read into a heap buffer of exactly its length.  Lookups are parsed from that
// buffer; entries reach cidr.h as the std::string its interface takes, copied from the buffer.
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "cidr.h"

using mxpcidr::u128;

static int hexval(int c) {
    if (c >= '0' && c <= '9') return c - '0';
    if (c >= 'a' && c <= 'f') return c - 'a' + 10;
    return -1;
}

static void print128(u128 v) { printf("%016" PRIx64 "%016" PRIx64, (uint64_t)(v >> 64), (uint64_t)v); }

struct List {
    std::vector<int> e_ok, o_ok;
    std::vector<std::pair<uint32_t, uint32_t>> r4;
    std::vector<std::pair<u128, u128>> r6;
    std::vector<std::pair<std::unique_ptr<uint8_t[]>, size_t>> lookups;
};

static void finish(List& L) {
    uint64_t n = 0;
    for (int ok : L.e_ok) {
        printf("E %d\n", ok);
        n += (uint64_t)ok;
    }
    for (int ok : L.o_ok) {
        printf("O %d\n", ok);
        n += (uint64_t)ok;
    }
    printf("N %" PRIu64 "\n", n);
    mxpcidr::merge(L.r4);
    mxpcidr::merge(L.r6);
    std::vector<uint32_t> lo4;
    for (auto& p : L.r4) {
        printf("4 %u %u\n", p.first, p.second);
        lo4.push_back(p.first);
    }
    for (auto& p : L.r6) {
        printf("6 ");
        print128(p.first);
        printf(" ");
        print128(p.second);
        printf("\n");
    }
    const std::vector<uint32_t> dir = mxpcidr::v4_directory(lo4);
    for (size_t k = 0; k < dir.size(); k++)
        if (k == 0 || dir[k] != dir[k - 1]) printf("D %zu %u\n", k, dir[k]);
    if (dir.size() != 65537) printf("D size %zu\n", dir.size());
    for (auto& q : L.lookups) {
        uint8_t ip[16];
        int r = -1;
        if (mxpnet::parse_ip(q.first.get(), (uint32_t)q.second, ip)) {
            r = 0;
            if (mxpnet::is_v4(ip)) {
                const uint32_t x = (uint32_t)ip[12] << 24 | (uint32_t)ip[13] << 16 | (uint32_t)ip[14] << 8 | ip[15];
                for (auto& p : L.r4)
                    if (p.first <= x && x <= p.second) r = 1;
            } else {
                u128 x = 0;
                for (int i = 0; i < 16; i++) x = x << 8 | ip[i];
                for (auto& p : L.r6)
                    if (p.first <= x && x <= p.second) r = 1;
            }
        }
        printf("L %d\n", r);
    }
    printf("=\n");
}

int main() {
    std::string line;
    List L;
    int c;
    bool more = true;
    while (more) {
        line.clear();
        while ((c = getchar()) != EOF && c != '\n') line.push_back((char)c);
        if (c == EOF) {
            if (line.empty()) break;
            more = false;
        }
        const char tag = line.empty() ? '?' : line[0];
        if (tag == '=' && line.size() == 1) {
            finish(L);
            L = List();
            continue;
        }
        if ((tag != 'e' && tag != 'o' && tag != 'l') || line.size() % 2 == 0) {
            fprintf(stderr, "bad line\n");
            return 2;
        }
        const size_t n = (line.size() - 1) / 2;
        std::unique_ptr<uint8_t[]> s(new uint8_t[n]);  // exact size: no byte behind the string
        for (size_t i = 0; i < n; i++) {
            const int hi = hexval(line[1 + 2 * i]), lo = hexval(line[2 + 2 * i]);
            if (hi < 0 || lo < 0) {
                fprintf(stderr, "bad hex line\n");
                return 2;
            }
            s[i] = (uint8_t)(hi * 16 + lo);
        }
        if (tag == 'l') {
            L.lookups.emplace_back(std::move(s), n);
        } else {
            const bool ok = mxpcidr::add_entry(std::string((const char*)s.get(), n), L.r4, L.r6, nullptr);
            (tag == 'e' ? L.e_ok : L.o_ok).push_back(ok ? 1 : 0);
        }
    }
    return 0;
}
