/*
 * bwts_unpack -- the inverse of bwts_pack: reads frames (include/bwts_pack.h) until the file ends, checks each, and writes the bytes
 * they hold, so concatenated frames unpack to the concatenated inputs.
 *
 *   bwts_unpack [-r <offset>:<bytes>]... <infile> [<outfile>]
 *   no outfile: the bytes go to standard output
 *   -r, which may be repeated: only bytes [offset, offset + bytes) of the unpacked file are written, the ranges one behind the other
 *       in the order given; only the blocks they touch are decoded and checked (bwts_unpack_ranges).  Offsets count in the whole
 *       unpacked file: a range that crosses from one frame into the next is read in two parts.  A range beyond the file is an error,
 *       and nothing is written.
 *   any error: a message on stderr, exit 1; a frame whose bytes fail their checksum gets a message of its own
 * The output is opened once the first frame has been unpacked and checked; with -r, once every range has been read.
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

static void usage(void)
{
	fprintf(stderr, "Usage: bwts_unpack [-r <offset>:<bytes>]... <infile> [<outfile>]\n");
	fprintf(stderr, "If unspecified, output is written to standard output\n");
	exit(1);
}

static void *need(size_t bytes)
{
	void *p = malloc(bytes ? bytes : 1);

	if (!p) {
		fprintf(stderr, "bwts_unpack: no memory for %llu bytes\n", (unsigned long long)bytes);
		exit(1);
	}
	return p;
}

/* <offset>:<bytes>, both decimal */
static int parse_range(const char *arg, bwts_range *r)
{
	char *end;
	unsigned long long v;

	if (*arg < '0' || *arg > '9')
		return 0;
	v = strtoull(arg, &end, 10);
	if (*end != ':' || end[1] < '0' || end[1] > '9')
		return 0;
	r->offset = v;
	v = strtoull(end + 1, &end, 10);
	r->bytes = v;
	return *end == 0;
}

/* The ranges of the unpacked file, frame by frame: every frame gets the parts of the ranges that lie in it in one call, and the
 * parts go to their places in the output, which is written when all of it is there. */
static uint64_t unpack_ranges(bwts_ctx *ctx, const unsigned char *in, uint64_t in_total, const bwts_range *ranges, uint64_t count,
			      unsigned char **out_bytes, double *device_ms, bwts_timings *t)
{
	uint64_t at = 0, start = 0, total = 0, sum = 0, i, k;
	uint64_t *dst = need((size_t)count * sizeof *dst), *place = need((size_t)count * sizeof *place);
	bwts_range *part = need((size_t)count * sizeof *part);
	unsigned char *out, *tmp;
	int rc;

	/* the file's unpacked length, from headers and directories alone */
	while (at < in_total) {
		uint64_t n = 0, frame_bytes = 0;

		if ((rc = bwts_unpack_size(in + at, in_total - at, &n, &frame_bytes)) != BWTS_OK)
			fail_at("not a frame", at, rc);
		total += n;
		at += frame_bytes;
	}
	for (i = 0; i < count; i++) {
		if (ranges[i].bytes == 0 || ranges[i].bytes > total || ranges[i].offset > total - ranges[i].bytes) {
			fprintf(stderr, "bwts_unpack: range %llu:%llu is empty or lies beyond the %llu bytes of the unpacked file\n",
				(unsigned long long)ranges[i].offset, (unsigned long long)ranges[i].bytes, (unsigned long long)total);
			exit(1);
		}
		dst[i] = sum;
		sum += ranges[i].bytes;
	}
	out = need((size_t)sum);
	tmp = need((size_t)sum);
	for (at = 0; at < in_total; ) {
		uint64_t n = 0, frame_bytes = 0, got = 0, parts = 0, from = 0;

		if ((rc = bwts_unpack_size(in + at, in_total - at, &n, &frame_bytes)) != BWTS_OK)
			fail_at("not a frame", at, rc);
		/* what of every range lies in [start, start + n) */
		for (i = 0; i < count; i++) {
			const uint64_t lo = ranges[i].offset > start ? ranges[i].offset : start;
			const uint64_t end = ranges[i].offset + ranges[i].bytes, hi = end < start + n ? end : start + n;

			if (lo >= hi)
				continue;
			part[parts].offset = lo - start;
			part[parts].bytes = hi - lo;
			place[parts++] = dst[i] + (lo - ranges[i].offset);
		}
		if (parts) {
			if ((rc = bwts_unpack_ranges(ctx, in + at, frame_bytes, part, parts, tmp, sum, &got)) != BWTS_OK)
				fail_at("reading ranges failed", at, rc);
			bwts_last_timings(ctx, t);
			*device_ms += t->total_ms;
			for (k = 0; k < parts; k++) {
				memcpy(out + place[k], tmp + from, (size_t)part[k].bytes);
				from += part[k].bytes;
			}
		}
		start += n;
		at += frame_bytes;
	}
	free(tmp);
	free(part);
	free(place);
	free(dst);
	*out_bytes = out;
	return sum;
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
	bwts_range *ranges = NULL;
	uint64_t nranges = 0;

	marks.main_start = cli_now_s();
	marks.write_s = 0.0;
	while (argc > 1 && strcmp(argv[1], "-r") == 0) {
		if (argc < 3)
			usage();
		if (!ranges)
			ranges = need((size_t)argc * sizeof *ranges);
		if (!parse_range(argv[2], &ranges[nranges++])) {
			fprintf(stderr, "bwts_unpack: a range is <offset>:<bytes>, two decimal numbers, not '%s'\n", argv[2]);
			exit(1);
		}
		argv += 2;
		argc -= 2;
	}
	if (argc < 2 || argc > 3)
		usage();
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
	if (nranges) {
		uint64_t got = unpack_ranges(ctx, in, in_total, ranges, nranges, &out, &device_ms, &t);
		double t0;

		fp = out_name ? fopen(out_name, "wb") : stdout;
		if (!fp) {
			fprintf(stderr, "Couldn't open output file for writing\n");
			perror(out_name);
			exit(1);
		}
		t0 = cli_now_s();
		if (fwrite(out, 1, (size_t)got, fp) != (size_t)got) {
			perror("write");
			exit(1);
		}
		marks.write_s += cli_now_s() - t0;
		out_total = got;
		at = in_total;
	}
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
	free(ranges);
	bwts_ctx_destroy(ctx);
	marks.destroyed = cli_now_s();
	if (show)
		cli_report_process(stderr, &marks);
	return 0;
}
