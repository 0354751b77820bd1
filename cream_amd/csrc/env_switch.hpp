// env_switch.hpp — a process-wide integer switch (kernel A/B runs): its initial value comes from the environment, read once
// on first use; a C-ABI setter changes it afterwards.  Plain C++ (block_seq.cpp is not compiled as HIP).
#pragma once
#include <stdlib.h>

#include <atomic>

namespace cream {
struct EnvSwitch {
    const char* env;                 // variable that sets the initial value
    int dflt;                        // value when the variable is not set
    int (*norm)(int) = nullptr;      // maps the environment's and the setter's values onto the valid ones (optional)
    std::atomic<int> v{-1};          // -1: environment not read yet

    int normalise(int x) const { return norm ? norm(x) : x; }
    int get()
    {
        int m = v.load(std::memory_order_relaxed);
        if (m < 0) {
            const char* e = getenv(env);
            m = e ? normalise(atoi(e)) : dflt;
            v.store(m, std::memory_order_relaxed);
        }
        return m;
    }
    // returns the previous value; x < 0 only asks
    int set(int x)
    {
        const int prev = get();
        if (x >= 0) v.store(normalise(x), std::memory_order_relaxed);
        return prev;
    }
};
inline int norm_bool(int x) { return x != 0; }
}  // namespace cream
