"""csrc/lrnde_buf.hpp on the host: the owners of device memory, pinned memory and events, compiled with
LRNDE_BUF_HOST_TEST against malloc-backed stand-ins for the HIP calls they make, under AddressSanitizer and UBSan.  The
program counts live allocations, can make the next allocation fail, and exits non-zero at the first broken claim."""
import os, subprocess, textwrap
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = textwrap.dedent(r'''
    #include <cstdio>
    #include <cstdlib>
    #include <cstring>
    #include <type_traits>
    #include <utility>
    // ---- the HIP calls the header makes, on the host heap ----
    enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2 };
    enum { hipHostMallocMapped = 2, hipEventDisableTiming = 2 };
    typedef struct ev_* hipEvent_t;
    static int live = 0, live_ev = 0, fail_next = 0, n_alloc = 0;
    static hipError_t sticky = hipSuccess;
    static hipError_t get(void** p, size_t bytes) {
      if (fail_next) { fail_next = 0; *p = (void*)0x1;   /* a failed call may leave garbage behind */
                       return sticky = hipErrorOutOfMemory; }
      *p = malloc(bytes ? bytes : 1); ++live; ++n_alloc; return hipSuccess;
    }
    static hipError_t put(void* p) { free(p); --live; return hipSuccess; }
    static hipError_t hipMalloc(void** p, size_t bytes) { return get(p, bytes); }
    static hipError_t hipFree(void* p) { return put(p); }
    static unsigned last_flags = 0;
    static hipError_t hipHostMalloc(void** p, size_t bytes, unsigned flags) { last_flags = flags; return get(p, bytes); }
    static hipError_t hipHostFree(void* p) { return put(p); }
    static hipError_t hipHostGetDevicePointer(void** d, void* h, unsigned) { *d = h; return hipSuccess; }
    static hipError_t hipGetLastError() { hipError_t e = sticky; sticky = hipSuccess; return e; }
    static hipError_t hipEventCreate(hipEvent_t* e) { *e = (hipEvent_t)malloc(1); ++live_ev; return hipSuccess; }
    static hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return hipEventCreate(e); }
    static hipError_t hipEventDestroy(hipEvent_t e) { free(e); --live_ev; return hipSuccess; }
    #define LRNDE_BUF_HOST_TEST
    #include "lrnde_buf.hpp"

    #define REQUIRE(x) do { if (!(x)) { fprintf(stderr, "line %d: %s\n", __LINE__, #x); exit(1); } } while (0)

    static_assert(!std::is_copy_constructible<DevBuf<float>>::value && !std::is_copy_assignable<DevBuf<float>>::value, "DevBuf copies");
    static_assert(!std::is_copy_constructible<PinBuf<int>>::value && !std::is_copy_assignable<PinBuf<int>>::value, "PinBuf copies");
    static_assert(!std::is_copy_constructible<HipEvent>::value && !std::is_copy_assignable<HipEvent>::value, "HipEvent copies");
    static_assert(std::is_nothrow_move_constructible<DevBuf<float>>::value && std::is_nothrow_move_assignable<PinBuf<int>>::value, "moves");

    template <class Buf> static void growth_verbs() {
      const int live0 = live;
      {
        Buf b;
        REQUIRE(b.get() == nullptr && b.size() == 0 && !b);
        // grow: keeps when n <= size(), replaces when larger
        REQUIRE(b.grow(8) == hipSuccess && b.size() == 8 && b.get() && live == live0 + 1);
        b.get()[7] = 1;   // (all 8 elements are there: ASan would see a short block)
        auto* p8 = b.get();
        int a = n_alloc;
        REQUIRE(b.grow(8) == hipSuccess && b.grow(3) == hipSuccess && b.grow(0) == hipSuccess);
        REQUIRE(b.get() == p8 && b.size() == 8 && n_alloc == a);
        REQUIRE(b.grow(9) == hipSuccess && b.size() == 9 && n_alloc == a + 1 && live == live0 + 1);
        b.get()[8] = 1;
        // a failed allocation leaves it empty (the old block is gone, the failed call's garbage is not kept) ...
        fail_next = 1;
        REQUIRE(b.grow(100) != hipSuccess && b.get() == nullptr && b.size() == 0 && live == live0);
        (void)hipGetLastError();
        // ... and a later grow succeeds
        REQUIRE(b.grow(4) == hipSuccess && b.size() == 4 && live == live0 + 1);
        // resize_exact: on any other n, a smaller one too; not on the same n
        a = n_alloc;
        REQUIRE(b.resize_exact(4) == hipSuccess && n_alloc == a);
        REQUIRE(b.resize_exact(2) == hipSuccess && b.size() == 2 && n_alloc == a + 1 && live == live0 + 1);
        REQUIRE(b.resize_exact(6) == hipSuccess && b.size() == 6 && n_alloc == a + 2 && live == live0 + 1);
        fail_next = 1;
        REQUIRE(b.resize_exact(7) != hipSuccess && !b && b.size() == 0 && live == live0);
        (void)hipGetLastError();
        // once: allocates when empty and never again
        a = n_alloc;
        REQUIRE(b.once(5) == hipSuccess && b.size() == 5 && n_alloc == a + 1);
        auto* p5 = b.get();
        REQUIRE(b.once(50) == hipSuccess && b.once(1) == hipSuccess && b.get() == p5 && b.size() == 5 && n_alloc == a + 1);
        fail_next = 1;
        Buf e;
        REQUIRE(e.once(5) != hipSuccess && !e && e.size() == 0);
        (void)hipGetLastError();
        REQUIRE(e.once(5) == hipSuccess && e.size() == 5);
        // reset empties; the pointer converts implicitly for the argument fillers
        auto* raw = static_cast<decltype(b.get())>(b);
        REQUIRE(raw == p5);
        REQUIRE(b.reset() == hipSuccess && !b && b.size() == 0);
        REQUIRE(b.reset() == hipSuccess);
      }
      REQUIRE(live == live0);
    }

    template <class Buf> static void moves() {
      const int live0 = live;
      {
        Buf a;
        REQUIRE(a.grow(4) == hipSuccess);
        auto* pa = a.get();
        Buf b(std::move(a));   // move construction transfers
        REQUIRE(!a && a.size() == 0 && b.get() == pa && b.size() == 4 && live == live0 + 1);
        Buf c;
        REQUIRE(c.grow(2) == hipSuccess && live == live0 + 2);
        c = std::move(b);      // move assignment frees the target's old block
        REQUIRE(!b && c.get() == pa && c.size() == 4 && live == live0 + 1);
        Buf& self = c;
        c = std::move(self);
        REQUIRE(c.get() == pa && c.size() == 4 && live == live0 + 1);
        REQUIRE(a.grow(1) == hipSuccess && live == live0 + 2);   // a moved-from buffer is an empty one
      }
      REQUIRE(live == live0);
    }

    int main() {
      growth_verbs<DevBuf<float>>();
      growth_verbs<PinBuf<int>>();
      growth_verbs<DevBuf<double>>();
      moves<DevBuf<float>>();
      moves<PinBuf<int>>();
      {  // try_grow: false on failure, empty, and the sticky error is cleared
        DevBuf<float> h;
        REQUIRE(h.try_grow(16) && h.size() == 16);
        REQUIRE(h.try_grow(8) && h.size() == 16);
        fail_next = 1;
        REQUIRE(!h.try_grow(1u << 20) && !h && h.size() == 0 && live == 0);
        REQUIRE(sticky == hipSuccess && hipGetLastError() == hipSuccess);
        REQUIRE(h.try_grow(32) && h.size() == 32);
      }
      REQUIRE(live == 0);
      {  // borrow: the alias frees nothing, whichever of the two goes first
        DevBuf<float>* owner = new DevBuf<float>();
        REQUIRE(owner->once(10) == hipSuccess);
        {
          DevBuf<float> alias;
          alias.borrow(*owner);
          REQUIRE(alias.get() == owner->get() && alias.size() == 10 && live == 1);
        }                                   // alias first
        REQUIRE(live == 1);
        owner->get()[9] = 2.f;              // (still the owner's: ASan would see a use after free)
        DevBuf<float>* alias = new DevBuf<float>();
        alias->borrow(*owner);
        delete owner;                       // owner first
        REQUIRE(live == 0);
        delete alias;
        REQUIRE(live == 0);
        // an alias that had a block of its own gives it up; one that is moved stays an alias; one that allocates owns again
        DevBuf<float> o, a;
        REQUIRE(o.once(3) == hipSuccess && a.once(3) == hipSuccess && live == 2);
        a.borrow(o);
        REQUIRE(live == 1 && a.get() == o.get());
        DevBuf<float> m(std::move(a));
        REQUIRE(m.get() == o.get() && m.reset() == hipSuccess && live == 1);
        a.borrow(o);
        REQUIRE(a.grow(20) == hipSuccess && a.get() != o.get() && live == 2);
      }
      REQUIRE(live == 0);
      {  // PinBuf: the flags reach the allocation; a mapped block keeps its device view, any other has none
        PinBuf<int> p;
        REQUIRE(p.once(16) == hipSuccess && last_flags == 0 && p.dev() == nullptr);
        PinBuf<int> q;
        REQUIRE(q.grow(16, hipHostMallocMapped) == hipSuccess && last_flags == hipHostMallocMapped && q.dev() == q.get());
        PinBuf<int> r(std::move(q));
        REQUIRE(r.dev() == r.get() && r.dev() && q.dev() == nullptr);
        REQUIRE(r.reset() == hipSuccess && r.dev() == nullptr);
      }
      REQUIRE(live == 0);
      {  // HipEvent: created once, destroyed if set
        HipEvent never;
        HipEvent e, f;
        REQUIRE((hipEvent_t)e == nullptr);
        REQUIRE(e.create() == hipSuccess && live_ev == 1 && (hipEvent_t)e != nullptr);
        hipEvent_t first = e;
        REQUIRE(e.create(hipEventDisableTiming) == hipSuccess && live_ev == 1 && (hipEvent_t)e == first);
        REQUIRE(f.create(hipEventDisableTiming) == hipSuccess && live_ev == 2);
      }
      REQUIRE(live_ev == 0);
      REQUIRE(live == 0);
      puts("ok");
      return 0;
    }
''')


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("buf")
    src = d / "t.cpp"
    src.write_text(SRC)
    exe = d / "t"
    subprocess.run(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-Wall", "-Werror",
                    "-Wno-unused-function", "-I", os.path.join(ROOT, "localregneuralde.jl_amd", "csrc"), str(src), "-o", str(exe)],
                   check=True)
    return str(exe)


def test_owners_on_the_host(program):
    r = subprocess.run([program], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_a_copy_does_not_compile(tmp_path):
    """a context copied wholesale would free its buffers twice: the owners make that a compile error"""
    head = SRC[:SRC.index("#define REQUIRE")]
    for body in ("DevBuf<float> a, b; b = a;", "DevBuf<float> a; DevBuf<float> b(a);", "PinBuf<int> a, b; b = a;",
                 "struct Ctx { DevBuf<float> w; }; Ctx a; Ctx b = a;"):
        src = tmp_path / "c.cpp"
        src.write_text(head + "int main() { " + body + " return 0; }\n")
        r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "localregneuralde.jl_amd", "csrc"), str(src)],
                           capture_output=True, text=True)
        assert r.returncode != 0 and "delete" in r.stderr, (body, r.stderr)
