// candidate_batch.h — the host image and the device block layout of a batch of candidate
// waypoint sets (host_candidates.cpp's CandidateBatch).  Host code only, no device call, so
// tests/candidate_layout_host.cpp runs it without a device.
#pragma once
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <vector>

#include "epp/types.h"
#include "host_waypoints.h"

namespace epp {

// `count` elements of T at byte `off` of the block.
template <class T>
struct Part {
    size_t off = 0, count = 0;
    size_t bytes() const { return count * sizeof(T); }
};

// The upload's host image [waypoints | offsets] of the sets and the layout of their device
// block.  The parts every call needs -- waypoints, segment times, coefficients, offsets, the
// fit's status -- are reserved here, a call's own outputs with part<T>() before the one
// allocation.  Every part starts 256-byte aligned (the kernels' wide loads of the times and
// the coefficients rest on that); a part of no elements is legal and takes no room.
struct CandidateLayout {
    size_t n = 0, total = 0, nseg = 0;  // sets, waypoints and segments of all sets
    size_t bytes = 0;                   // the block so far (a multiple of 256)
    std::vector<double> wp;             // total x 3
    std::vector<int32_t> off;           // n + 1: set k's waypoints are off[k] .. off[k + 1] - 1
    Part<double> p_wp, p_T, p_C;
    Part<int32_t> p_off, p_fit;

    explicit CandidateLayout(const std::vector<std::vector<Vec3>>& sets) : n(sets.size()), off(sets.size() + 1, 0) {
        for (const auto& s : sets)
            if (s.size() < 2) throw std::invalid_argument("At least two waypoints are required");
        for (size_t k = 0; k < n; ++k) {
            flatten(sets[k], wp);
            off[k + 1] = (int32_t)(wp.size() / 3);
        }
        total = wp.size() / 3;
        nseg = total - n;
        p_wp = part<double>(total * 3);
        p_T = part<double>(nseg);
        p_C = part<double>(nseg * 30);
        p_off = part<int32_t>(n + 1);
        p_fit = part<int32_t>(n);
    }

    template <class T>
    Part<T> part(size_t count) {
        auto after = [](size_t o, size_t b) { return (o + b + 255) & ~(size_t)255; };  // 256-B aligned parts
        const Part<T> p{bytes, count};
        bytes = after(bytes, p.bytes());
        return p;
    }
    // Set k's segments in the time and coefficient parts: [seg_begin(k), seg_begin(k + 1)).
    size_t seg_begin(size_t k) const { return (size_t)off[k] - k; }
};

}  // namespace epp
