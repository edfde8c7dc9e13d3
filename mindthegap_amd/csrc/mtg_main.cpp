/*
 * mtg_main.cpp -- the `MindTheGap` executable: module dispatch of /root/reference/src/main.cpp:62-124.
 * `fill` is complete; of `find`, the reference's other module, the homozygous insertions are built (`find -homo-insertions`).
 * `profile` is this build's own: the data access underneath `find` (a reference genome's k-mers against the graph), without its classification.
 */
#include "../../include/mtg_fill.h"
#include <cstdio>
#include <cstring>

int main(int argc, char** argv)
{
    if (argc < 2 || strcmp(argv[1], "-help") == 0 || strcmp(argv[1], "-h") == 0) {
        printf("\nMindTheGap (mindthegap_amd build: fill module on MI355X)\nUsage:\n   MindTheGap fill (-in <reads.fq> | -graph <graph>) (-bkpt <breakpoints.fa> | -contig <contigs.fa>) [options]\n   MindTheGap find (-in <reads.fq> | -graph <graph>) -ref <genome.fa> -homo-insertions [options]\n   MindTheGap -version\n");
        return 1;
    }
    if (strcmp(argv[1], "-version") == 0 || strcmp(argv[1], "-v") == 0) { printf("MindTheGap version 2.3.0 (mindthegap_amd, HIP gfx950)\n"); return 0; }
    if (strcmp(argv[1], "fill") == 0) return mtg_fill_main(argc - 2, (const char* const*)(argv + 2));
    if (strcmp(argv[1], "profile") == 0) return mtg_profile_main(argc - 2, (const char* const*)(argv + 2));
    if (strcmp(argv[1], "find") == 0) return mtg_find_main(argc - 2, (const char* const*)(argv + 2));
    fprintf(stderr, "EXCEPTION: unknown module '%s'\n", argv[1]);
    return 1;
}
