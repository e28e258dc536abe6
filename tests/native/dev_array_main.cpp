// Stand-alone check of the array type that the design handles own their device memory with (adelie_amd/csrc/dev_array_host.hpp),
// built with -fsanitize=address,undefined by tests/test_dev_array_host.py.  OwnedArr runs on a malloc/free policy that can be told
// to refuse; after every step the program prints "<step> <bytes owned>", and the Python side compares the numbers.  A block freed
// twice, used after its release or never freed is the sanitizers' to report.
#include "../../adelie_amd/csrc/dev_array_host.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>

using namespace ahip;

struct HostMem {
    static int& refuse_after() { static int k = -1; return k; } // -1: never; k: the (k + 1)-th request from now is refused
    static void* alloc(size_t bytes) {
        if (refuse_after() == 0) return nullptr;
        if (refuse_after() > 0) --refuse_after();
        return std::malloc(bytes ? bytes : 1);
    }
    static void free(void* p) { std::free(p); }
};
template <class T> using Arr = OwnedArr<T, HostMem>;

static void say(const char* step) { std::printf("%s %lld\n", step, (long long)owned_arr_bytes().load()); }

// what a design handle is to the type: several arrays in one object
struct Handle {
    Arr<double> a;
    Arr<int32_t> b;
    Arr<void> c;
    Arr<uint8_t> d;
    void build() { a.alloc(10), b.alloc(6), c.alloc(33), d.alloc(5); }
};

int main() {
    say("start");
    {
        Arr<double> a;
        a.alloc(37);
        std::memset(a.get(), 0, 37 * sizeof(double)); // (every byte of the block is ours)
        say("alloc");
    }
    say("destroyed");
    {
        Arr<void> v;
        v.alloc(13); // void counts bytes
        say("alloc_void");
        const double* as_double = static_cast<const double*>(v);
        if ((const void*)as_double != v.get()) return 3;
    }
    {
        Arr<int64_t> a;
        HostMem::refuse_after() = 0;
        const bool ok = a.try_alloc(5);
        HostMem::refuse_after() = -1;
        if (ok || a.get() != nullptr || a) return 4;
        say("try_alloc_refused");
        bool threw = false;
        HostMem::refuse_after() = 0;
        try { a.alloc(5); } catch (const core_error&) { threw = true; }
        HostMem::refuse_after() = -1;
        if (!threw || a.get() != nullptr) return 5;
        say("alloc_refused");
        a.alloc(5);
        HostMem::refuse_after() = 0;
        if (a.try_alloc(7) || a.get() != nullptr) return 6; // a refused request leaves the array empty, the old block freed
        HostMem::refuse_after() = -1;
        say("try_alloc_refused_over_owner");
    }
    {
        Arr<float> a;
        a.alloc(8);
        float* p = a.get();
        Arr<float> b(std::move(a));
        if (a.get() != nullptr || b.get() != p) return 7;
        say("move_construct");
        Arr<float> c;
        c.alloc(3);
        say("second_owner");
        c = std::move(b); // frees c's 12 bytes, takes b's 32
        if (b.get() != nullptr || c.get() != p) return 8;
        say("move_assign");
        Arr<float>& self = c;
        c = std::move(self);
        if (c.get() != p) return 9;
        c[0] = 1.0f; // (still alive)
        say("self_move");
    }
    say("moved_destroyed");
    {
        double raw[4] = {1, 2, 3, 4};
        Arr<double> owner;
        owner.alloc(4);
        {
            Arr<double> br, bo;
            br.borrow(raw);
            bo.borrow(owner);
            if (br.get() != raw || bo.get() != owner.get()) return 10;
            say("borrowed");
            Arr<double> had;
            had.alloc(2);
            had.borrow(raw + 1); // a borrow over an owned block frees the block
            say("borrow_over_owner");
            Arr<double> moved(std::move(bo)); // a moved borrower still owns nothing
            if (moved.get() != owner.get()) return 11;
        }
        say("borrowers_destroyed");
        owner.get()[3] = raw[3]; // the lender's block outlived them
        owner.borrow(owner);     // (a no-op, not a release)
        if (!owner.get()) return 12;
        say("self_borrow");
    }
    {
        Arr<uint16_t> a;
        a.alloc(9);
        a.reset();
        say("reset");
        a.reset();
        say("reset_twice");
        if (a.get() != nullptr) return 13;
    }
    {
        bool threw = false;
        try {
            Handle h;
            HostMem::refuse_after() = 2; // a and b succeed, c is refused
            try { h.build(); } catch (...) { HostMem::refuse_after() = -1; say("struct_alloc_threw"); throw; }
        } catch (const core_error& e) {
            threw = std::strstr(e.what(), "33 bytes") != nullptr;
        }
        if (!threw) return 14;
        say("struct_destroyed");
    }
    say("end");
    return 0;
}
