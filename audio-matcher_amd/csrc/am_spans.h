// am_spans.h -- which parts of a host haystack a per-hit call stages: the union of the hits' sample ranges, laid out
// one merged span after the other.  Standard library only (tests/test_hit_spans_host.py builds it with g++).
#pragma once
#include <algorithm>
#include <cstddef>
#include <numeric>
#include <vector>

namespace am {

struct HitRange { size_t lo, hi; };   // the elements [lo, hi) one hit reads, lo <= hi
struct Span { size_t lo, hi, off; };  // a merged span [lo, hi) and where its copy starts, in elements

// The ranges of n hits (in the call's order) merged where they overlap or touch (a range joins the span before it when
// its lo <= that span's hi: a gap of one element keeps two spans) into `spans`, ascending, each with its running
// offset; span_of[i]: the span that holds hit i.  Returns the total of staged elements.
inline size_t merge_spans(const HitRange* r, size_t n, std::vector<Span>& spans, std::vector<size_t>& span_of) {
    std::vector<size_t> order(n);
    std::iota(order.begin(), order.end(), (size_t)0);
    std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return r[a].lo < r[b].lo; });
    spans.clear();
    span_of.resize(n);
    size_t staged = 0;
    for (size_t i : order) {
        if (!spans.empty() && r[i].lo <= spans.back().hi) {
            staged += std::max(r[i].hi, spans.back().hi) - spans.back().hi;
            spans.back().hi = std::max(r[i].hi, spans.back().hi);
        } else {
            spans.push_back({r[i].lo, r[i].hi, staged});
            staged += r[i].hi - r[i].lo;
        }
        span_of[i] = spans.size() - 1;
    }
    return staged;
}

}  // namespace am
