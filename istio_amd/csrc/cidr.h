// cidr.h -- the host half of an IP_ADDRESSES list (lists.cpp): parseIPList / addEntry
// (ipList.go:35-75) on net.ParseCIDR, and the tables the device searches: the IPNets as disjoint,
// merged, sorted address intervals per family (IPNet.Contains per family after To4), plus the /16
// directory of the IPv4 intervals.  Host only: nothing from HIP or the engine, so the tests compile
// it into a stand-alone program (tests/cidr_host.cpp).
#pragma once

#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <limits>
#include <string>
#include <utility>
#include <vector>

#include "netparse.h"

namespace mxpcidr {

typedef unsigned __int128 u128;

// net.ParseCIDR (Go 1.9 src/net/ip.go) -> IPNet{IP: ip.Mask(m), Mask: m}; false on ParseError
struct Net {
    uint8_t ip[16];
    int iplen;
    uint8_t mask[16];
    int masklen;
};

inline bool parse_cidr(const std::string& s, Net* out) {
    const size_t slash = s.find('/');
    if (slash == std::string::npos) return false;
    const uint8_t* a = (const uint8_t*)s.data();
    uint8_t ip[16];
    int iplen = 4;
    if (!mxpnet::parse_v4(a, (uint32_t)slash, ip)) {
        iplen = 16;
        if (!mxpnet::parse_v6(a, (uint32_t)slash, ip)) return false;
    }
    int n;
    uint32_t used;
    const uint8_t* m = a + slash + 1;
    const uint32_t ml = (uint32_t)(s.size() - slash - 1);
    if (!mxpnet::dtoi(m, ml, &n, &used) || used != ml || n < 0 || n > 8 * iplen) return false;
    // CIDRMask(n, 8 * iplen)
    uint8_t mask[16] = {0};
    for (int i = 0; i < iplen; i++) {
        const int bits = std::min(8, std::max(0, n - 8 * i));
        mask[i] = (uint8_t)(0xFF00u >> bits);
    }
    // ip.Mask(m): a 4-byte mask on a v4-in-v6 address masks its last 4 bytes
    Net r{};
    r.masklen = iplen;
    memcpy(r.mask, mask, iplen);
    const uint8_t* src = ip;
    int srclen = 16;
    if (iplen == 4 && mxpnet::is_v4(ip)) {
        src = ip + 12;
        srclen = 4;
    }
    if (srclen != iplen) return false;  // not reachable from ParseCIDR
    r.iplen = iplen;
    for (int i = 0; i < iplen; i++) r.ip[i] = src[i] & mask[i];
    *out = r;
    return true;
}

// networkNumberAndMask (ip.go): the family a net matches after IP.To4, or false (never matches)
inline bool net_number_and_mask(const Net& n, uint8_t nn[16], int* nnlen, uint8_t m[16]) {
    uint8_t ip16[16];
    const uint8_t* ip = n.ip;
    int iplen = n.iplen;
    if (iplen == 16 && mxpnet::is_v4(n.ip)) {  // To4 of a v4-in-v6 network number
        memcpy(ip16, n.ip + 12, 4);
        ip = ip16;
        iplen = 4;
    }
    const uint8_t* mk = n.mask;
    int mlen = n.masklen;
    if (mlen == 4) {
        if (iplen != 4) return false;
    } else if (mlen == 16) {
        if (iplen == 4) {
            mk = n.mask + 12;
            mlen = 4;
        }
    } else {
        return false;
    }
    memcpy(nn, ip, iplen);
    memcpy(m, mk, mlen);
    *nnlen = iplen;
    return true;
}

template <class T>
void merge(std::vector<std::pair<T, T>>& v) {
    std::sort(v.begin(), v.end());
    std::vector<std::pair<T, T>> o;
    for (auto& p : v) {
        if (!o.empty() && (p.first <= o.back().second || (o.back().second != std::numeric_limits<T>::max() &&
                                                          p.first == o.back().second + 1)))
            o.back().second = std::max(o.back().second, p.second);
        else
            o.push_back(p);
    }
    v.swap(o);
}

// addEntry (ipList.go:61-75): "/32" appended when the entry has no '/' (*full: the text ParseCIDR
// saw, for the error message), then the net's address range pushed into its family's vector (none
// for an IPNet that contains nothing).  False: ParseCIDR refused the entry.
inline bool add_entry(const std::string& orig, std::vector<std::pair<uint32_t, uint32_t>>& r4,
                      std::vector<std::pair<u128, u128>>& r6, std::string* full) {
    std::string ip = orig;
    if (ip.find('/') == std::string::npos) ip += "/32";
    if (full) *full = ip;
    Net n;
    if (!parse_cidr(ip, &n)) return false;
    uint8_t nn[16], m[16];
    int len;
    if (!net_number_and_mask(n, nn, &len, m)) return true;  // an IPNet that contains nothing
    if (len == 4) {
        uint32_t lo = 0, mm = 0;
        for (int i = 0; i < 4; i++) {
            lo = lo << 8 | (uint32_t)(nn[i] & m[i]);
            mm = mm << 8 | m[i];
        }
        r4.emplace_back(lo, lo | ~mm);
    } else {
        u128 lo = 0, mm = 0;
        for (int i = 0; i < 16; i++) {
            lo = lo << 8 | (u128)(nn[i] & m[i]);
            mm = mm << 8 | m[i];
        }
        r6.emplace_back(lo, lo | ~mm);
    }
    return true;
}

// /16 directory of the IPv4 intervals: dir[k] = intervals whose start is below k << 16
inline std::vector<uint32_t> v4_directory(const std::vector<uint32_t>& lo4) {
    std::vector<uint32_t> dir(65537, 0);
    for (uint32_t k = 0, i = 0; k <= 65536; k++) {
        const uint64_t at = (uint64_t)k << 16;
        while (i < lo4.size() && lo4[i] < at) i++;
        dir[k] = i;
    }
    return dir;
}

}  // namespace mxpcidr
