// Serial stand-in for the three pieces of the Parallel Patterns Library the
// reference codec names (test infrastructure only; see oracle/Makefile).
// Everything runs in the calling thread, in order: the pinned path is the
// serial build(false), so nothing here ever needs to be concurrent.
#pragma once
#include <functional>

namespace concurrency {

template <typename Index, typename Fn>
void parallel_for(Index first, Index last, const Fn& fn) {
    for (Index i = first; i < last; ++i) fn(i);
}

template <typename F1, typename F2>
void parallel_invoke(const F1& f1, const F2& f2) {
    f1();
    f2();
}

template <typename T>
class combinable {
public:
    template <typename Init>
    explicit combinable(Init init) : value_(init()) {}
    T& local() { return value_; }
    template <typename Op>
    T combine(Op) const { return value_; }

private:
    T value_;
};

}  // namespace concurrency
