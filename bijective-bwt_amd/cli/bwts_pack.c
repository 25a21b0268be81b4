/*
 * bwts_pack -- compress a file on the GPU: bijective BWT, move-to-front and rANS over blocks, one checksummed frame
 * (include/bwts_pack.h) per 2^32 input bytes.
 *
 *   bwts_pack [-z] [-p <2|4|8>] [-b <KiB>] <infile> [<outfile>]
 *   -b <KiB>: block size in KiB, at least 4 (default: every frame is one block)
 *   -z: frames of version 2, zero-run coding between move-to-front and the coder
 *   -p <width>: frames of version 3 for arrays of 2-, 4- or 8-byte numbers: every block split into byte planes in front of the
 *      transform; implies -z
 *   the options come in any order
 *   no outfile: the frames go to standard output
 *   any error: a message on stderr, exit 1
 * The output is opened once the first frame exists, so a failing run leaves no truncated destination behind.
 * BWTS_TIMINGS=1 prints where the time went, like mk_bwts.
 */
#define _GNU_SOURCE
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bwts_pack.h"
#include "map_file.h"
#include "cli_report.h"

#define FRAME_INPUT_MAX (1ull << 32)

static void usage(void)
{
	fprintf(stderr, "Usage: bwts_pack [-z] [-p <2|4|8>] [-b <KiB>] <infile> [<outfile>]\n");
	fprintf(stderr, "-b: block size in KiB, at least 4 (default: one block per frame)\n");
	fprintf(stderr, "-z: zero-run coding in front of the coder (frame version 2)\n");
	fprintf(stderr, "-p: byte planes of 2-, 4- or 8-byte numbers in front of the transform (frame version 3; implies -z)\n");
	fprintf(stderr, "If unspecified, output is written to standard output\n");
	exit(1);
}

static void fail(const char *what, int code)
{
	fprintf(stderr, "bwts_pack: %s: %s\n", what, bwts_strerror(code));
	exit(1);
}

int main(int argc, char **argv)
{
	unsigned char *text, *out;
	long len;
	bwts_ctx *ctx;
	bwts_timings t;
	FILE *fp = NULL;
	int rc, arg = 1;
	uint64_t block_bytes = 0, at, in_total, out_total = 0, cap;
	uint32_t version = 1, width = 0;
	double device_ms = 0.0;
	const char *dev = getenv("BWTS_DEVICE"), *show_env = getenv("BWTS_TIMINGS"), *out_name;
	const int show = show_env && show_env[0] == '1';
	struct cli_marks marks;

	marks.main_start = cli_now_s();
	marks.write_s = 0.0;
	while (arg < argc && (strcmp(argv[arg], "-b") == 0 || strcmp(argv[arg], "-z") == 0 || strcmp(argv[arg], "-p") == 0)) {
		char *end = NULL;
		unsigned long long kib;

		if (argv[arg][1] == 'z') {
			version = 2;
			arg++;
			continue;
		}
		if (argc < arg + 2)
			usage();
		if (argv[arg][1] == 'p') {
			kib = strtoull(argv[arg + 1], &end, 10);
			if (!end || *end || (kib != 2 && kib != 4 && kib != 8)) {
				fprintf(stderr, "bwts_pack: the width of a number must be 2, 4 or 8 bytes\n");
				exit(1);
			}
			width = (uint32_t)kib;
			arg += 2;
			continue;
		}
		kib = strtoull(argv[arg + 1], &end, 10);
		if (!end || *end || kib < 4 || kib > (1ull << 22)) {
			fprintf(stderr, "bwts_pack: block size must be 4 .. 4194304 KiB\n");
			exit(1);
		}
		block_bytes = (uint64_t)kib << 10;
		arg += 2;
	}
	if (argc - arg < 1 || argc - arg > 2)
		usage();
	out_name = argc - arg == 2 ? argv[arg + 1] : NULL;
	map_in(text, len, argv[arg]);
	marks.mapped = cli_now_s();
	in_total = (uint64_t)len;

	if ((rc = bwts_ctx_create(&ctx, dev ? atoi(dev) : 0)) != BWTS_OK)
		fail("cannot open GPU context", rc);
	marks.ctx_ready = cli_now_s();
	cap = width ? bwts_pack_planes_bound(width, in_total < FRAME_INPUT_MAX ? in_total : FRAME_INPUT_MAX, block_bytes)
		    : bwts_pack_bound_v(version, in_total < FRAME_INPUT_MAX ? in_total : FRAME_INPUT_MAX, block_bytes);
	out = cap ? malloc(cap) : NULL;
	if (!out) {
		fprintf(stderr, "bwts_pack: no memory for a frame of up to %llu bytes\n", (unsigned long long)cap);
		exit(1);
	}
	for (at = 0; at < in_total; at += FRAME_INPUT_MAX) {
		const uint64_t n = in_total - at < FRAME_INPUT_MAX ? in_total - at : FRAME_INPUT_MAX;
		uint64_t bytes = 0;
		double t0;

		rc = width ? bwts_pack_planes(ctx, width, text + at, n, block_bytes, out, cap, &bytes)
			   : bwts_pack_v(ctx, version, text + at, n, block_bytes, out, cap, &bytes);
		if (rc != BWTS_OK)
			fail("packing failed", rc);
		bwts_last_timings(ctx, &t);
		device_ms += t.total_ms;
		if (!fp) {
			fp = out_name ? fopen(out_name, "wb") : stdout;
			if (!fp) {
				fprintf(stderr, "Couldn't open output file for writing\n");
				perror(out_name);
				exit(1);
			}
		}
		t0 = cli_now_s();
		if (fwrite(out, 1, (size_t)bytes, fp) != (size_t)bytes) {
			perror("write");
			exit(1);
		}
		marks.write_s += cli_now_s() - t0;
		out_total += bytes;
	}
	if ((fp != stdout ? fclose(fp) : fflush(fp)) != 0) {
		perror("write");
		exit(1);
	}
	marks.done = cli_now_s();
	if (show) {
		fprintf(stderr, "Packed %llu bytes into %llu (%0.4f)  device time %0.3f  fwrite %0.3f\n", (unsigned long long)in_total,
			(unsigned long long)out_total, (double)out_total / (double)in_total, 1e-3 * device_ms, marks.write_s);
		cli_report_host_costs(stderr, &t);
	}
	free(out);
	bwts_ctx_destroy(ctx);
	marks.destroyed = cli_now_s();
	if (show)
		cli_report_process(stderr, &marks);
	return 0;
}
