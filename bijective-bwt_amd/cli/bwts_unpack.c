/*
 * bwts_unpack -- the inverse of bwts_pack: reads frames (include/bwts_pack.h) until the file ends, checks each, and writes the bytes
 * they hold, so concatenated frames unpack to the concatenated inputs.
 *
 *   bwts_unpack <infile> [<outfile>]
 *   no outfile: the bytes go to standard output
 *   any error: a message on stderr, exit 1; a frame whose bytes fail their checksum gets a message of its own
 * The output is opened once the first frame has been unpacked and checked.
 */
#define _GNU_SOURCE
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bwts_pack.h"
#include "map_file.h"
#include "cli_report.h"

static void fail_at(const char *what, uint64_t at, int code)
{
	if (code == BWTS_E_CHECKSUM)
		fprintf(stderr, "bwts_unpack: CHECKSUM MISMATCH in the frame at offset %llu: the data is damaged, nothing of this frame was written\n",
			(unsigned long long)at);
	else
		fprintf(stderr, "bwts_unpack: %s (frame at offset %llu): %s\n", what, (unsigned long long)at, bwts_strerror(code));
	exit(1);
}

int main(int argc, char **argv)
{
	unsigned char *in, *out = NULL;
	long len;
	bwts_ctx *ctx;
	bwts_timings t;
	FILE *fp = NULL;
	int rc;
	uint64_t at = 0, in_total, out_total = 0, out_cap = 0;
	double device_ms = 0.0;
	const char *dev = getenv("BWTS_DEVICE"), *show_env = getenv("BWTS_TIMINGS"), *out_name;
	const int show = show_env && show_env[0] == '1';
	struct cli_marks marks;

	marks.main_start = cli_now_s();
	marks.write_s = 0.0;
	if (argc < 2 || argc > 3) {
		fprintf(stderr, "Usage: bwts_unpack <infile> [<outfile>]\n");
		fprintf(stderr, "If unspecified, output is written to standard output\n");
		exit(1);
	}
	out_name = argc == 3 ? argv[2] : NULL;
	map_in(in, len, argv[1]);
	marks.mapped = cli_now_s();
	in_total = (uint64_t)len;

	if ((rc = bwts_ctx_create(&ctx, dev ? atoi(dev) : 0)) != BWTS_OK) {
		fprintf(stderr, "bwts_unpack: cannot open GPU context: %s\n", bwts_strerror(rc));
		exit(1);
	}
	marks.ctx_ready = cli_now_s();
	memset(&t, 0, sizeof t);
	while (at < in_total) {
		uint64_t n = 0, frame_bytes = 0, got = 0;
		double t0;

		if ((rc = bwts_unpack_size(in + at, in_total - at, &n, &frame_bytes)) != BWTS_OK)
			fail_at("not a frame", at, rc);
		if (n > out_cap) {
			free(out);
			out = malloc((size_t)n);
			out_cap = n;
			if (!out) {
				fprintf(stderr, "bwts_unpack: no memory for %llu bytes\n", (unsigned long long)n);
				exit(1);
			}
		}
		if ((rc = bwts_unpack(ctx, in + at, frame_bytes, out, out_cap, &got)) != BWTS_OK)
			fail_at("unpacking failed", at, rc);
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
		if (fwrite(out, 1, (size_t)got, fp) != (size_t)got) {
			perror("write");
			exit(1);
		}
		marks.write_s += cli_now_s() - t0;
		out_total += got;
		at += frame_bytes;
	}
	if ((fp != stdout ? fclose(fp) : fflush(fp)) != 0) {
		perror("write");
		exit(1);
	}
	marks.done = cli_now_s();
	if (show) {
		fprintf(stderr, "Unpacked %llu bytes from %llu  device time %0.3f  fwrite %0.3f\n", (unsigned long long)out_total,
			(unsigned long long)in_total, 1e-3 * device_ms, marks.write_s);
		cli_report_host_costs(stderr, &t);
	}
	free(out);
	bwts_ctx_destroy(ctx);
	marks.destroyed = cli_now_s();
	if (show)
		cli_report_process(stderr, &marks);
	return 0;
}
