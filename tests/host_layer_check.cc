// host_layer_check.cc -- the host layer's two pieces of plain C++ as a program of its own, for the sanitizers (tests/test_host_layer.py
// builds it with -fsanitize=thread and with -fsanitize=address,undefined, and runs it as a child process): the copy workers of
// copy_pool.h, with 1 and with 6 parts, and the arithmetic of seg_layout.h.
#include "copy_pool.h"
#include "seg_layout.h"

#include <stdio.h>
#include <stdlib.h>

static int failures = 0, checks = 0;
#define CHECK(cond, ...) do { checks++; if (!(cond)) { failures++; printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

static const size_t MiB = (size_t)1 << 20, PAGE = 4096;

static char *map_pages(size_t bytes, int prot)
{
    void *p = mmap(nullptr, (bytes + PAGE - 1) & ~(PAGE - 1), prot, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (p == MAP_FAILED) { printf("mmap of %zu bytes failed\n", bytes); exit(2); }
    return (char *)p;
}

static void copies(CopyPool &pool, const char *src_block, char *dst_block)
{
    const size_t sizes[] = {0, 1, 4095, MiB - 1, MiB, MiB + 4097, 9 * MiB + 1}, offs[] = {0, 1, 4095};
    for (size_t n : sizes)
        for (size_t so : offs)
            for (size_t dof : offs) {
                const char *src = src_block + so;
                char *dst = dst_block + PAGE + dof;                  // a guard byte in front of dst and one behind it
                memset(dst - 1, 0xAA, n + 2);
                pool.copy(dst, src, n);
                CHECK(memcmp(dst, src, n) == 0, "copy of %zu bytes, offsets %zu -> %zu, %d parts: bytes differ", n, so, dof, pool.parts);
                CHECK((unsigned char)dst[-1] == 0xAA && (unsigned char)dst[n] == 0xAA, "copy of %zu bytes, offsets %zu -> %zu, %d parts: a guard byte changed", n, so, dof,
                      pool.parts);
            }
}

// pages of a fresh anonymous mapping, every third one filled first: pre-faulting must leave all of them as they are
static void touches(CopyPool &pool, const char *src_block)
{
    struct { size_t bytes, start; } cases[] = {{4 * MiB - 1, 0}, {4 * MiB, 0}, {13 * MiB + 123, 777}};
    for (const auto &c : cases) {
        const size_t room = c.start + c.bytes;
        char *m = map_pages(room, PROT_READ | PROT_WRITE), *want = (char *)calloc(room, 1);
        for (size_t pg = 0; pg * PAGE + PAGE <= room; pg += 3) {
            memset(m + pg * PAGE, (int)(pg % 251) + 1, PAGE);
            memset(want + pg * PAGE, (int)(pg % 251) + 1, PAGE);
        }
        pool.touch_async(m + c.start, c.bytes);
        pool.wait();
        CHECK(!pool.touching, "touching still set after wait()");
        CHECK(memcmp(m, want, room) == 0, "pre-faulting %zu bytes from offset %zu changed them (%d parts)", c.bytes, c.start, pool.parts);
        // the next job is a copy again
        pool.copy(m + c.start, src_block, 2 * MiB + 5);
        CHECK(memcmp(m + c.start, src_block, 2 * MiB + 5) == 0, "the copy behind a pre-fault did not copy (%d parts)", pool.parts);
        CHECK(memcmp(m + c.start + 2 * MiB + 5, want + c.start + 2 * MiB + 5, c.bytes - 2 * MiB - 5) == 0, "the copy behind a pre-fault went too far (%d parts)", pool.parts);
        free(want);
        munmap(m, (room + PAGE - 1) & ~(PAGE - 1));
    }
    // a mapping the kernel will not populate for writing: the job ends, and says so
    char *ro = map_pages(8 * MiB, PROT_READ);
    pool.touch_async(ro, 8 * MiB);
    pool.wait();
    CHECK(pool.parts == 1 ? !pool.touch_failed.load() : pool.touch_failed.load(), "touch_failed after a refused populate, %d parts", pool.parts);
    CHECK(ro[0] == 0 && ro[8 * MiB - 1] == 0, "read-only pages changed");
    munmap(ro, 8 * MiB);
}

static void pool_checks(int parts)
{
    const size_t room = 9 * MiB + 3 * PAGE;
    char *src = map_pages(room, PROT_READ | PROT_WRITE), *dst = map_pages(room, PROT_READ | PROT_WRITE);
    for (size_t i = 0; i < room; i += 8) { const uint64_t v = i * 0x9E3779B97F4A7C15ull + 1; memcpy(src + i, &v, 8); }
    CopyPool pool;
    pool.start(parts);
    CHECK(pool.parts == parts && (int)pool.workers.size() == parts - 1, "%d parts asked for, %d made", parts, pool.parts);
    copies(pool, src, dst);
    touches(pool, src);
    for (int k = 0; k < 300; k++) {                  // jobs in quick succession, the two kinds in turn
        if (k & 1) { pool.touch_async(dst, 4 * MiB); pool.wait(); }
        else {
            pool.copy(dst + (k % 7), src + (k % 5), MiB + (size_t)k);
            CHECK(memcmp(dst + (k % 7), src + (k % 5), MiB + (size_t)k) == 0, "job %d: bytes differ (%d parts)", k, parts);
        }
    }
    pool.shutdown();
    CHECK(pool.workers.empty(), "workers left after shutdown");
    munmap(src, room);
    munmap(dst, room);
}

static void layout_checks()
{
    const uint64_t counts[] = {1, 2, 3, 255, 256, (uint64_t)1 << 20};
    for (uint64_t c : counts) {
        const uint64_t room_words = seg_room_bytes(c) / 8;
        CHECK(seg_room_bytes(c) == (24 * (c + 1) + 65535) / 65536 * 65536, "room for %llu segments", (unsigned long long)c);
        CHECK(seg_offset_words(c) == c + 1 && seg_upload_at(c) == c + 1 && seg_dir_at(c) == c + 1, "regions of %llu segments start behind the offsets", (unsigned long long)c);
        CHECK(seg_upload_at(c) + seg_upload_max_words(c) <= room_words && seg_upload_max_words(c) == 2 * c + 1, "upload of %llu segments", (unsigned long long)c);
        CHECK(seg_dir_at(c) + seg_dir_words(c) <= room_words && seg_dir_words(c) == 2 * c, "directory of %llu blocks", (unsigned long long)c);
        CHECK(seg_readback_at(c) + seg_readback_words(c) <= room_words && seg_readback_words(c) * 8 >= c * 4, "read-back of %llu segments", (unsigned long long)c);
        // the checksum's upload of c + 1 words and its read-back are live together
        CHECK(seg_readback_at(c) >= seg_upload_at(c) + (c + 1), "read-back of %llu segments lies on the checksum's upload", (unsigned long long)c);
    }
}

int main()
{
    pool_checks(1);
    pool_checks(6);
    layout_checks();
    if (failures) { printf("%d of %d checks FAILED\n", failures, checks); return 1; }
    printf("%d checks ok\n", checks);
    return 0;
}
